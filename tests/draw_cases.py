"""The annotation of the source frame (cf_draw_faces / cf_op_draw, csrc/cf_draw.hip, csrc/cf_drawmath.h) restated in numpy, and the
cases the device is held to.  The statement (include/centerface_hip.h has it in full): a row's box and landmarks are mapped to frame
pixels in float64 (fixed order, no FMA), floor, clamped to [-8192, 16384]; outline, dots, plate and ink are sets of frame pixels with a
layer each (1 held, 2 live, 3 ink, 4 dot); a pixel takes the colour of the highest layer any row puts on it; a chroma sample that of the
highest layer over its four luma pixels; undrawn bytes are not written.

Options are spelled as ``_lib.draw_opts`` takes them, always in full (``OPT`` and ``opt(...)``), so that the restatement owns no
default.  ``Frames`` is the pitched / dense buffer helper of tests/test_redact.py (padding and guard bands pre-filled with PAD)."""
import numpy as np

from test_redact import Frames, pitches_for                                # noqa: F401  (re-exported for the tests)

BOX, LANDMARKS = 1, 2
LABELS = {"none": 0, "score": 1, "id": 2}
GLYPH = ((0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E), (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
         (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E), (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
         (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08), (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
         (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C))
# [digit][row][col] -> ink, col 0 = the left column = bit 4
GLYPH_BITS = np.array([[[(row >> (4 - col)) & 1 for col in range(5)] for row in g] for g in GLYPH], bool)

OPT = dict(what=BOX | LANDMARKS, thickness=1, radius=2, label="score", label_scale=1, dash_held=1, scale=1.0,
           box_color=(2, 255, 0), held_color=(0, 255, 255), lm_color=(0, 0, 255), text_color=(10, 20, 30))


def opt(**kw):
    o = dict(OPT)
    o.update(kw)
    return o


def yuv_color_ref(bgr):
    """Integer BT.601 limited range, >> 8 as floor division (python's >> floors)."""
    b, g, r = (int(v) for v in bgr)
    return (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128)


def yuv_opt(o):
    """The same options with the four colours converted for a 4:2:0 frame."""
    return dict(o, **{k: yuv_color_ref(o[k]) for k in ("box_color", "held_color", "lm_color", "text_color")})


# ------------------------------------------------------------------------------------------ the restatement
def point(v, f):
    return int(min(max(np.floor(np.float64(v) * np.float64(f)), -8192.0), 16384.0))


def draw_layout_ref(o, box, score, lms, info, h, w, H, W):
    """int32 [32] as cf_draw_layout: ok, X1, Y1, X2, Y2, held, plate x0, y0, Pw, Ph, n, digits[10], valid bits, Lx0, Ly0 .. Lx4, Ly4."""
    out = np.zeros(32, np.int64)
    x1, y1, x2, y2 = (np.float64(np.float32(v)) for v in box)
    s = np.float64(np.float32(o["scale"]))
    t, k, label = int(o["thickness"]), int(o["label_scale"]), LABELS.get(o["label"], o["label"])
    if not (np.isfinite(x1) and np.isfinite(y1) and np.isfinite(x2) and np.isfinite(y2)):
        return out.astype(np.int32)
    cx, cy = (x1 + x2) * 0.5, (y1 + y2) * 0.5
    hw, hh = (x2 - x1) * 0.5 * s, (y2 - y1) * 0.5 * s
    if not (hw > 0 and hh > 0):
        return out.astype(np.int32)
    fx, fy = np.float64(w) / np.float64(W), np.float64(h) / np.float64(H)
    out[0] = 1
    out[1], out[2], out[3], out[4] = point(cx - hw, fx), point(cy - hh, fy), point(cx + hw, fx), point(cy + hh, fy)
    out[5] = 1 if info is not None and int(info[2]) > 0 else 0
    if lms is not None:
        for j in range(5):
            lx, ly = np.float64(np.float32(lms[2 * j])), np.float64(np.float32(lms[2 * j + 1]))
            if np.isfinite(lx) and np.isfinite(ly):
                out[21] |= 1 << j
                out[22 + 2 * j], out[23 + 2 * j] = point(lx, fx), point(ly, fy)
    value = None
    if label == 1:
        sc = np.float64(np.float32(score))
        if np.isfinite(sc):
            value = int(min(max(np.floor(sc * np.float64(100.0)), 0.0), 100.0))
    elif label == 2 and info is not None and int(info[0]) > 0:
        value = int(info[0])
    if value is not None:
        digits = [int(c) for c in str(value)]
        n = len(digits)
        out[10] = n
        out[11:11 + n] = digits
        out[8], out[9] = k * (6 * n + 1), 9 * k
        out[6] = out[1]
        out[7] = out[2] - out[9] if out[2] - out[9] >= 0 else out[2] + t
    return out.astype(np.int32)


def row_layers(rec, o, h, w):
    """uint8 [h, w]: the layer one row's record puts on every frame pixel."""
    L = np.zeros((h, w), np.uint8)
    if not rec[0]:
        return L
    rec = [int(v) for v in rec]
    y, x = np.mgrid[0:h, 0:w]
    t, r, k, what = int(o["thickness"]), int(o["radius"]), int(o["label_scale"]), int(o["what"])
    X1, Y1, X2, Y2, held = rec[1:6]
    base = 1 if held else 2
    if what & BOX:
        m = (x >= X1) & (x <= X2) & (y >= Y1) & (y <= Y2) & ((x < X1 + t) | (x > X2 - t) | (y < Y1 + t) | (y > Y2 - t))
        if held and int(o["dash_held"]):
            m &= ((x + y) % (8 * t)) < 4 * t
        L[m] = base
    x0, y0, Pw, Ph, n = rec[6:11]
    if n > 0:
        plate = (x >= x0) & (x < x0 + Pw) & (y >= y0) & (y < y0 + Ph)
        L[plate] = np.maximum(L[plate], base)
        u, v = (x - x0) // k, (y - y0) // k
        q, col = (u - 1) // 6, (u - 1) % 6
        cell = plate & (v >= 1) & (v <= 7) & (u >= 1) & (q < n) & (col < 5)
        digit = np.array(rec[11:21])[np.clip(q, 0, 9)]
        ink = cell & GLYPH_BITS[digit, np.clip(v - 1, 0, 6), np.clip(col, 0, 4)]
        L[ink] = 3
    if (what & LANDMARKS) and not held:
        for j in range(5):
            if rec[21] >> j & 1:
                dx, dy = x - rec[22 + 2 * j], y - rec[23 + 2 * j]
                L[dx * dx + dy * dy <= r * r + r] = 4
    return L


def image_layers(o, boxes, scores, lms, info, h, w, H, W):
    """uint8 [h, w]: the highest layer over the rows of one image."""
    L = np.zeros((h, w), np.uint8)
    for i in range(len(boxes)):
        rec = draw_layout_ref(o, boxes[i], scores[i], None if lms is None else lms[i], None if info is None else info[i], h, w, H, W)
        L = np.maximum(L, row_layers(rec, o, h, w))
    return L


def paint(views, fmt, L, o):
    """Writes the colours of the layer map L into one frame's row views (tests/test_redact.py's Frames.views), drawn bytes only."""
    lut = np.zeros((5, 3), np.uint8)
    for layer, name in ((1, "held_color"), (2, "box_color"), (3, "text_color"), (4, "lm_color")):
        lut[layer] = o[name]
    h, w = L.shape
    m = L > 0
    if fmt == "bgr":
        for ch in range(3):
            views[0][:, ch::3][m] = lut[L, ch][m]
        return
    views[0][m] = lut[L, 0][m]
    C = L.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))
    cm = C > 0
    c1, c2 = (2, 1) if fmt in ("nv21", "yv12") else (1, 2)                # plane order: memory order of the two chroma channels
    if fmt in ("nv12", "nv21"):
        views[1][:, 0::2][cm] = lut[C, c1][cm]
        views[1][:, 1::2][cm] = lut[C, c2][cm]
    else:
        views[1][cm] = lut[C, c1][cm]
        views[2][cm] = lut[C, c2][cm]


def draw_ref(views, fmt, boxes, scores, counts, net_hw, h, w, lms=None, info=None, **o):
    """The restatement of ops.draw_faces on the row views of B frames, in place; returns the per-image layer maps."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32).reshape(-1)
    lms = None if lms is None else np.asarray(lms, np.float32).reshape(-1, 10)
    info = None if info is None else np.asarray(info, np.int32).reshape(-1, 3)
    maps, at = [], 0
    for b, n in enumerate(int(c) for c in counts):
        sl = slice(at, at + n)
        L = image_layers(o, boxes[sl], scores[sl], None if lms is None else lms[sl], None if info is None else info[sl], h, w, *net_hw)
        paint(views[b], fmt, L, o)
        maps.append(L)
        at += n
    return maps


# ------------------------------------------------------------------------------------------ the rows and the cases
NAN, INF = float("nan"), float("inf")


def standard_rows(h, w, H, W):
    """The rows of one image, designed in FRAME pixels and divided into the network's coordinates: boxes straddling each frame edge and
    the paint kernel's tile edges (y = 16, 32; x = 64 where the frame is wider), one fully outside, one thinner than 2t for t >= 3, two
    overlapping live boxes, a held box over a live one with crossing plates, dots on the frame border and outside it, a non-finite
    landmark, two skipped rows.  Returns (boxes [N,4], scores [N], lms [N,10], info [N,3])."""
    fx, fy = w / W, h / H
    far = (w + 40.0, h + 40.0)
    rows = [
        # frame-pixel box,                    score, id, misses, five landmark points (frame pixels)
        ((-5, 5, 10, 20),                     0.05,  7, 0, [(0, 0), (3, 12), (-3, 10), far, (2, 19)]),
        ((20, -6, 34, 8),                     0.42,  42, 0, [(22, 0), (30, 2), (27, -9), (NAN, 3), (33, 7)]),
        ((w - 8, 10, w + 6, 30),              1.0,   2147483647, 0, [(w - 1, 12), (w + 1, 20), (w - 4, 25), (w - 2, INF), (w - 6, 29)]),
        ((30, h - 6, 45, h + 5),              0.999, 3, 0, [(32, h - 1), (40, h - 3), (44, h + 2), (36, h - 5), (31, h - 2)]),
        ((w + 10, h + 10, w + 30, h + 30),    0.7,   4, 0, [far] * 5),
        ((12, 24, 15.5, 40),                  0.3,   0, 0, [(13, 26), (14, 30), (13, 33), (14, 36), (13, 39)]),
        ((18, 12, 40, 30),                    0.61,  12, 0, [(24, 17), (34, 17), (29, 22), (25, 26), (33, 26)]),
        ((28, 20, 50, 38),                    0.87,  13, 0, [(34, 25), (44, 25), (39, 30), (35, 34), (43, 34)]),
        ((24, 14, 46, 34),                    0.5,   99, 2, [(30, 19), (40, 19), (35, 24), (31, 29), (39, 29)]),
        ((NAN, 5, 20, 20),                    0.9,   5, 0, [(10, 10)] * 5),
        ((22, 9, 22, 30),                     0.9,   6, 0, [(22, 10)] * 5),
        ((60, 2, 70, 14),                     0.25,  8, 1, [(62, 4), (66, 4), (64, 8), (62, 12), (66, 12)]),
        ((w - 20, h - 16, w - 2, h - 2),      NAN,   10, 0, [(w - 15, h - 12), (w - 7, h - 12), (w - 11, h - 8), (w - 14, h - 5), (w - 8, h - 5)]),
    ]
    boxes = np.float32([[b[0] / fx, b[1] / fy, b[2] / fx, b[3] / fy] for b, _, _, _, _ in rows])
    scores = np.float32([s for _, s, _, _, _ in rows])
    lms = np.float32([[v for px, py in pts for v in (px / fx, py / fy)] for _, _, _, _, pts in rows])
    info = np.int32([[i, 1, m] for _, _, i, m, _ in rows])
    return boxes, scores, lms, info


class Case(object):
    """One comparison: B frames of ``fmt`` (pitched unless ``dense``), packed rows, the network size and the options; ``layers``: all
    four layers must own a pixel of the expected frames."""

    def __init__(self, name, fmt, B, h, w, dense, rows, counts, net, o, layers=False, use_info=True):
        self.name, self.fmt, self.B, self.h, self.w, self.dense, self.net, self.layers = name, fmt, B, h, w, dense, net, layers
        self.boxes, self.scores, self.lms, self.info = rows
        if not use_info:
            self.info = None
        self.counts = np.asarray(counts, np.int32)
        self.o = o if fmt == "bgr" else yuv_opt(o)

    def frames(self, seed=13):
        p0, p1 = pitches_for(self.fmt, self.w)
        return Frames(np.random.default_rng(seed), self.fmt, self.B, self.h, self.w, p0, p1, self.dense)

    def expect(self, fr):
        """A clone of ``fr`` with the restatement applied, and the layer maps."""
        want = fr.clone()
        maps = draw_ref(want.views, self.fmt, self.boxes, self.scores, self.counts, self.net, self.h, self.w, lms=self.lms, info=self.info, **self.o)
        return want, maps

    def kwargs(self):
        return dict(fmt=self.fmt, lms=self.lms, info=self.info, **self.o)


def three_images(h, w, net):
    """Image 0: the standard rows; image 1: none; image 2: the standard rows reversed (another order, the same picture)."""
    b, s, l, i = standard_rows(h, w, *net)
    rows = tuple(np.concatenate([a, a[::-1]]) for a in (b, s, l, i))
    return rows, [len(b), 0, len(b)]


def many_boxes(n, h, w, seed=5):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-4, w, n), rng.uniform(-4, h, n)
    bw, bh = rng.uniform(2, 9, n), rng.uniform(2, 9, n)
    boxes = np.float32(np.stack([x, y, x + bw, y + bh], 1))
    lms = np.float32(rng.uniform(-4, max(h, w) + 4, (n, 10)))
    info = np.int32(np.stack([np.arange(1, n + 1), np.ones(n), rng.integers(0, 2, n)], 1))
    return boxes, np.float32(rng.uniform(0, 1, n)), lms, info


def cases():
    out = []
    net = (32, 48)                                                        # 48 x 64 frames: fx = 4/3, fy = 3/2
    rows, counts = three_images(48, 64, net)
    for fmt in ("bgr", "nv12", "nv21", "i420", "yv12"):
        for dense in (False, True):
            out.append(Case("%s-%s" % (fmt, "dense" if dense else "pitched"), fmt, 3, 48, 64, dense, rows, counts, net, opt(), layers=True))
    rows_odd, counts_odd = three_images(37, 51, (32, 48))
    out.append(Case("bgr-odd", "bgr", 3, 37, 51, False, rows_odd, counts_odd, (32, 48), opt(label="id"), layers=True))
    wide = {f: three_images(hh, ww, (40, 160)) for f, (hh, ww) in (("bgr", (33, 133)), ("nv12", (34, 134)), ("i420", (34, 134)))}
    for f, (hh, ww) in (("bgr", (33, 133)), ("nv12", (34, 134)), ("i420", (34, 134))):
        out.append(Case("%s-wide" % f, f, 3, hh, ww, False, wide[f][0], wide[f][1], (40, 160), opt(label="id", label_scale=2, thickness=3), layers=True))
    sweep = (
        ("t3-r0-id-s13-nodash", opt(thickness=3, radius=0, label="id", scale=1.3, dash_held=0), True),
        ("t16-k8-id", opt(thickness=16, label="id", label_scale=8), True),
        ("r16", opt(radius=16), False),                                       # the dots of thirteen rows cover most of a 48 x 64 frame
        ("box-only", opt(what=BOX, label="none"), False),
        ("dots-only", opt(what=LANDMARKS, label="none"), False),
        ("label-only", opt(what=0, label="score", label_scale=2), False),
        ("s13-score", opt(scale=1.3, thickness=3, label="score"), True),
    )
    for name, o, layers in sweep:
        for fmt in ("bgr", "nv12"):
            out.append(Case("%s-%s" % (fmt, name), fmt, 3, 48, 64, False, rows, counts, net, o, layers=layers))
    out.append(Case("bgr-untracked", "bgr", 3, 48, 64, False, rows, counts, net, opt(), use_info=False))      # info = None: all rows live
    # the smallest frames: one box over everything, a dot on pixel (0, 0)
    tiny = (np.float32([[0, 0, 8, 8]]), np.float32([0.5]), np.float32([[0, 0] * 5]), np.int32([[1, 1, 0]]))
    out.append(Case("nv12-2x2", "nv12", 1, 2, 2, False, tiny, [1], (2, 2), opt(label="none")))
    out.append(Case("bgr-2x2", "bgr", 1, 2, 2, False, tiny, [1], (2, 2), opt(label="none")))
    out.append(Case("bgr-1x1", "bgr", 1, 1, 1, False, tiny, [1], (1, 1), opt(label="none")))
    # more frames than one launch's plane table
    r33 = many_boxes(33 * 2, 16, 16, seed=9)
    out.append(Case("nv12-33-frames", "nv12", 33, 16, 16, False, r33, [2] * 33, (16, 16), opt(label="id")))
    # more rows than one 256-lane step of the tile's scan
    out.append(Case("bgr-300-rows", "bgr", 1, 64, 64, False, many_boxes(300, 64, 64), [300], (64, 64), opt(label="id", radius=1), layers=True))
    out.append(Case("i420-300-rows", "i420", 1, 64, 64, False, many_boxes(300, 64, 64), [300], (64, 64), opt(label="none", radius=1)))
    return out


CASES = cases()


def permuted(case, seed=3):
    """The same case with the rows of every image in another order."""
    rng = np.random.default_rng(seed)
    idx, at = [], 0
    for n in case.counts:
        idx.extend(at + rng.permutation(int(n)))
        at += int(n)
    idx = np.asarray(idx, np.int64)
    rows = (case.boxes[idx], case.scores[idx], case.lms[idx], None if case.info is None else case.info[idx])
    c = Case(case.name + "-permuted", case.fmt, case.B, case.h, case.w, case.dense, rows, case.counts, case.net, OPT, case.layers)
    c.o, c.info = case.o, rows[3]
    return c

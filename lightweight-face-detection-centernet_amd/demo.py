"""The evaluator-facing pieces of the reference's ``demo.py``: image files in (``cv2.imread`` at demo.py:31,74 ->
PIL here), the WIDER-FACE result-file format (``demo.py:81-87``) and a batched dump loop.  GUI/webcam/``cv2.imshow``
parts are out of scope."""
import os

import numpy as np


def imread(path):
    """``cv2.imread(path)`` (demo.py:31,74): uint8 [H, W, 3] in BGR channel order.  Decoded with PIL (cv2 is not
    a dependency); both sit on libjpeg, bit parity of the DECODER with a cv2 build is unpinned."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def detect_file(detector, path, threshold=0.3):
    """demo.py:30-38 (``test_image``): read one image file and run ``CenterFace.__call__`` on it.  ``detector`` must
    have been built for the image's (h, w) -- or be a ``CenterFaceBuckets``, which takes any size."""
    frame = imread(path)
    if hasattr(detector, "detect"):
        return detector.detect([frame], threshold)[0]
    return detector(frame, threshold)


def format_wider_result(rel_name, dets):
    """Text of one result file exactly as demo.py:82-87 writes it: image path, count, then
    ``x y w h score`` per box with w = x2 - x1 + 1, h = y2 - y1 + 1 (:86)."""
    lines = ['{:s}\n'.format(rel_name), '{:d}\n'.format(len(dets))]
    for b in dets:
        x1, y1, x2, y2, s = (float(v) for v in b[:5])
        lines.append('{:.1f} {:.1f} {:.1f} {:.1f} {:.3f}\n'.format(x1, y1, (x2 - x1 + 1), (y2 - y1 + 1), s))
    return ''.join(lines)


def write_wider_result(save_path, im_dir, im_name, dets):
    """demo.py:67-68,81-87: save_path/im_dir/im_name.txt."""
    d = os.path.join(save_path, im_dir)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, im_name + '.txt')
    with open(path, 'w') as f:
        f.write(format_wider_result('%s/%s.jpg' % (im_dir, im_name), dets))
    return path


def dump_event(detector, images, im_dir, names, save_path):
    """Detect a list of same-sized BGR uint8 images in batches with one ``CenterFace`` instance (the
    reference rebuilds the model per image, demo.py:76) and write one result file per image."""
    results = detector.detect_batch(images, threshold=0.05)
    paths = []
    for name, res in zip(names, results):
        dets = res[0] if isinstance(res, tuple) else res
        paths.append(write_wider_result(save_path, im_dir, name, dets))
    return paths


def _fit_detector(fit, dtype, flip=False):
    """The detector of ``fit=N``: an N x N context that takes a frame of any size letterboxed (``CenterFace.detect_fit``: the aspect
    ratio kept, black padding; no accuracy claim is made for it)."""
    from .centerface import CenterFace
    return CenterFace(fit, fit, dtype=dtype, flip_test=flip)


def _views_detector(frame, scales, tiled, dtype, flip=False, size=640, pack=False, gutter=0):
    """The detector, the frame and the ``views=`` options of ``scales=(1.0, 0.5)``: the image (cropped to even sides) goes through an
    N x N context -- N = ``tiled`` when tiles are asked for, else ``size`` -- as several views in one batch: N x N tiles first when
    ``tiled``, then the aspect-true whole image at each scale (``CenterFace.detect_views``; no accuracy claim is made for it).  ``pack``:
    the views share canvases (``ops.pack_views`` with ``gutter`` pixels of fill between them) instead of taking one each."""
    from . import ops
    from .centerface import CenterFace
    frame = np.ascontiguousarray(frame[:frame.shape[0] & ~1, :frame.shape[1] & ~1])
    n = int(tiled) if tiled else int(size)
    views = dict(scales=tuple(float(v) for v in scales), tile=int(tiled) if tiled else None)
    table = ops.view_layout(frame.shape[0], frame.shape[1], n, n, **views)
    V = ops.pack_views(table, 1, (n, n), int(gutter))[1] if pack else len(table)
    if pack:
        views.update(pack=True, gutter=int(gutter))
    return CenterFace(n, n, dtype=dtype, max_batch=V * (2 if flip else 1), flip_test=flip), frame, views


def _upright_hw(frame, rotate):
    """The (height, width) of the upright view of a stored frame that ``rotate`` clockwise degrees make upright."""
    return (frame.shape[1], frame.shape[0]) if rotate in (90, 270) else (frame.shape[0], frame.shape[1])


def anonymize_file(path, out_path, **options):
    """Read one image file, redact every detected face on the device (``CenterFace.anonymize``; ``options``: mode, shape, cell,
    scale, fill, or mode='blur' with shape, radius, scale) and write the result to ``out_path`` (format from its extension).  Returns the detections.  ``tiled=N``: sliced
    inference with N x N tiles at native resolution (``CenterFace.detect_tiled``; the image is cropped to even sides), for images much
    larger than N whose small faces a whole-frame resize would lose; the detections are then in image pixels.  ``fit=N``: the image
    goes letterboxed through an N x N context instead of one built for its size; not together with ``tiled``.  ``flip=True``: the
    detector runs CenterNet's flip test (``CenterFace(flip_test=True)``: about twice the network time; no accuracy claim is made).
    ``rotate=N`` (90, 180, 270): the image is STORED turned and N clockwise degrees make it upright -- the detector sees the upright
    view (``CenterFace.anonymize(rotate=)``), the faces are redacted in the image as stored; not together with ``tiled``.
    ``scales=(1.0, 0.5)``: multi-scale detection (``CenterFace.anonymize(views=)``) -- the whole image at each scale, behind the N x N
    tiles of ``tiled=N`` if given, as one batch through a 640 x 640 (N x N) context; not together with ``fit`` or ``rotate``.
    ``pack=True`` (``gutter=N``) beside ``scales``: the views share canvases (``CenterFace.detect_views(pack=True)``)."""
    from PIL import Image
    from .centerface import CenterFace
    frame = imread(path)
    tiled = int(options.pop("tiled", 0) or 0)
    fit = int(options.pop("fit", 0) or 0)
    dtype = options.pop("dtype", "bf16")
    flip = bool(options.pop("flip", False))
    rotate = options["rotate"] = int(options.pop("rotate", 0) or 0)
    scales, pack, gutter = options.pop("scales", None), options.pop("pack", False), options.pop("gutter", 0)
    if pack and not scales:
        raise ValueError("pack= goes with scales=")
    if scales:
        if fit or rotate:
            raise ValueError("scales= goes with tiled= only, not with fit= or rotate=")
        detector, frame, options["views"] = _views_detector(frame, scales, tiled, dtype, flip, pack=pack, gutter=gutter)
    elif fit:
        detector = _fit_detector(fit, dtype, flip)
        options["fit"], options["tiled"] = True, bool(tiled)
    elif tiled:
        from . import ops
        frame = np.ascontiguousarray(frame[:frame.shape[0] & ~1, :frame.shape[1] & ~1])
        T = len(ops.tile_grid(frame.shape[0], frame.shape[1], tiled, (tiled // 4) & ~1))
        detector = CenterFace(tiled, tiled, dtype=dtype, max_batch=T, flip_test=flip)
        options["tiled"] = True
    else:
        detector = CenterFace(*_upright_hw(frame, rotate), dtype=dtype, flip_test=flip)
    try:
        frames, results = detector.anonymize([frame], **options)
    finally:
        detector.close()
    Image.fromarray(np.ascontiguousarray(frames[0][:, :, ::-1])).save(out_path)
    return results[0]


def annotate_file(path, out_path, **options):
    """demo.py:30-51 (``test_image`` with its drawing loop): read one image file, draw every detection on the device
    (``CenterFace.annotate``: green boxes, red landmark dots, the score as a label; ``options`` as there) and write the result to
    ``out_path`` (format from its extension).  Returns the detections.  ``tiled=N``, ``fit=N``, ``flip=True``, ``rotate=N``, ``scales=``: as ``anonymize_file``
    (the labels are upright in the image as stored)."""
    from PIL import Image
    from .centerface import CenterFace
    frame = imread(path)
    tiled = int(options.pop("tiled", 0) or 0)
    fit = int(options.pop("fit", 0) or 0)
    dtype = options.pop("dtype", "bf16")
    flip = bool(options.pop("flip", False))
    rotate = options["rotate"] = int(options.pop("rotate", 0) or 0)
    scales, pack, gutter = options.pop("scales", None), options.pop("pack", False), options.pop("gutter", 0)
    if pack and not scales:
        raise ValueError("pack= goes with scales=")
    if scales:
        if fit or rotate:
            raise ValueError("scales= goes with tiled= only, not with fit= or rotate=")
        detector, frame, options["views"] = _views_detector(frame, scales, tiled, dtype, flip, pack=pack, gutter=gutter)
    elif fit:
        detector = _fit_detector(fit, dtype, flip)
        options["fit"], options["tiled"] = True, bool(tiled)
    elif tiled:
        from . import ops
        frame = np.ascontiguousarray(frame[:frame.shape[0] & ~1, :frame.shape[1] & ~1])
        T = len(ops.tile_grid(frame.shape[0], frame.shape[1], tiled, (tiled // 4) & ~1))
        detector = CenterFace(tiled, tiled, dtype=dtype, max_batch=T, flip_test=flip)
        options["tiled"] = True
    else:
        detector = CenterFace(*_upright_hw(frame, rotate), dtype=dtype, flip_test=flip)
    try:
        frames, results = detector.annotate([frame], **options)
    finally:
        detector.close()
    Image.fromarray(np.ascontiguousarray(frames[0][:, :, ::-1])).save(out_path)
    return results[0]


def chips_file(path, out_dir, size=112, tiled=0, dtype="bf16", fit=0, flip=False, rotate=0, scales=None, pack=False, gutter=0):
    """Read one image file and write the aligned chip of every detected face, cut from the image at its own resolution
    (``CenterFace.detect_aligned_frames``), to ``out_dir``/<image name>_<k>.png.  Returns (detections, the paths written).
    ``tiled=N``: sliced inference with N x N tiles (the image is cropped to even sides).  ``fit=N``, ``flip=True``, ``rotate=N``, ``scales=``: as ``anonymize_file``
    (the chips are fitted to the landmarks, so they come out upright)."""
    from PIL import Image
    from .centerface import CenterFace
    frame = imread(path)
    tiled, fit, rotate, views = int(tiled or 0), int(fit or 0), int(rotate or 0), None
    if scales:
        if fit or rotate:
            raise ValueError("scales= goes with tiled= only, not with fit= or rotate=")
        detector, frame, views = _views_detector(frame, scales, tiled, dtype, flip, pack=pack, gutter=gutter)
        tiled = 0
    elif fit:
        detector = _fit_detector(fit, dtype, flip)
    elif tiled:
        from . import ops
        frame = np.ascontiguousarray(frame[:frame.shape[0] & ~1, :frame.shape[1] & ~1])
        T = len(ops.tile_grid(frame.shape[0], frame.shape[1], tiled, (tiled // 4) & ~1))
        detector = CenterFace(tiled, tiled, dtype=dtype, max_batch=T, flip_test=flip)
    else:
        detector = CenterFace(*_upright_hw(frame, rotate), dtype=dtype, flip_test=flip)
    try:
        dets, lms, chips = detector.detect_aligned_frames(frame[None], "bgr", size, tiled=bool(tiled), fit=bool(fit) or None, rotate=rotate, views=views)[0]
    finally:
        detector.close()
    os.makedirs(out_dir, exist_ok=True)
    stem, paths = os.path.splitext(os.path.basename(path))[0], []
    for k, chip in enumerate(chips):
        paths.append(os.path.join(out_dir, "%s_%d.png" % (stem, k)))
        Image.fromarray(np.ascontiguousarray(chip[:, :, ::-1])).save(paths[-1])
    return (dets, lms), paths


def main(argv=None):
    """``python -m centerface_amd.demo IMAGE [--anonymize OUT | --chips DIR | --draw OUT] [--tiled N | --fit [N]] [--scales S,S.. [--pack [--gutter N]]] [--flip] [--rotate N]``: print the detections of one image
    file; with ``--draw`` also write the image with every detection drawn into it (boxes, landmark dots and, unless ``--label none``,
    the score); with
    ``--anonymize`` also write the image with every face pixelated (or blanked: ``--mode solid``; or blurred: ``--blur [R]``, R = the
    filter strength 1..24, without it or 0 an eighth of each face's smaller side); with ``--chips`` write one aligned
    ``--size`` x ``--size`` chip per face, cut from the image at its own resolution, into DIR; with ``--tiled N`` beside either the
    faces are found by sliced inference over N x N tiles at native resolution; with ``--fit [N]`` (default 640) the image goes through an
    N x N context letterboxed -- its aspect ratio kept, black padding, the detections mapped back into image pixels -- instead of a
    context built for its size (no accuracy claim is made for it); with ``--flip`` the detector runs CenterNet's flip test -- the image and
    its mirror in one forward, the heads merged on the device -- at about twice the network time (no accuracy claim is made either); with ``--rotate N``
    (90, 180 or 270) the image is taken as STORED turned, N clockwise degrees making it upright: the detector sees the upright view and
    the detections, the redaction and the drawing are in the pixels of the image as stored (not with ``--tiled``; no accuracy claim); with
    ``--scales 1,0.5`` the image goes through a 640 x 640 context (``--tiled N``: N x N, behind N x N tiles) as one batch of views -- the
    whole image, aspect ratio kept, at each scale -- whose detections are merged on the device (multi-scale detection; not with ``--fit``
    or ``--rotate``; one view per canvas; no accuracy claim is made); with ``--pack`` beside ``--scales`` the views are packed into shared
    canvases, ``--gutter N`` pixels of fill between them (``--scales 1,0.5,0.25`` of a 1080p image: one 640 x 640 canvas instead of three;
    the decode's NMS is then per canvas; the gutter default 0 is this project's choice, nobody has measured it)."""
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("image")
    ap.add_argument("--anonymize", metavar="OUT", help="write the image with every detected face redacted to OUT")
    ap.add_argument("--mode", default="mosaic", choices=("mosaic", "solid"))
    ap.add_argument("--shape", default="ellipse", choices=("ellipse", "rect"))
    ap.add_argument("--cell", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.3)
    ap.add_argument("--blur", type=int, nargs="?", const=0, default=None, metavar="R",
                    help="with --anonymize: blur the faces instead (R in 1..24; 0 or no value: per face, from its size)")
    ap.add_argument("--tiled", type=int, default=0, metavar="N", help="with --anonymize / --chips: detect on overlapping N x N tiles (N a multiple of 32)")
    ap.add_argument("--fit", type=int, nargs="?", const=640, default=0, metavar="N",
                    help="detect through an N x N context with the image letterboxed (N a multiple of 32; default 640)")
    ap.add_argument("--flip", action="store_true", help="flip test: run the image and its mirror and merge the heads on the device (about twice the network time)")
    ap.add_argument("--rotate", type=int, default=0, choices=(0, 90, 180, 270), metavar="N",
                    help="the image is stored turned: N clockwise degrees (90, 180, 270) make it upright; detect in the upright view")
    ap.add_argument("--scales", default=None, metavar="S,S..", type=lambda t: tuple(float(v) for v in t.split(",")),
                    help="multi-scale detection: the whole image at each of these fractions of its fitted size (e.g. 1,0.5), merged on the device")
    ap.add_argument("--pack", action="store_true", help="with --scales: pack the views into shared canvases instead of one canvas per view")
    ap.add_argument("--gutter", type=int, default=0, metavar="N", help="with --pack: N pixels of fill between packed views (default 0)")
    ap.add_argument("--chips", metavar="DIR", help="write the aligned chip of every detected face, cut from the image itself, into DIR")
    ap.add_argument("--size", type=int, default=112, help="with --chips: the chip side (a multiple of 4 in [16, 512])")
    ap.add_argument("--draw", metavar="OUT", help="write the image with every detection drawn into it to OUT")
    ap.add_argument("--label", default="score", choices=("score", "none"), help="with --draw: the number above each box")
    args = ap.parse_args(argv)
    if args.tiled and not (args.anonymize or args.chips or args.draw or args.scales):
        ap.error("--tiled goes with --anonymize, --chips, --draw or --scales")
    if args.scales and (args.fit or args.rotate):
        ap.error("--scales goes with --tiled only, not with --fit or --rotate")
    if args.pack and not args.scales:
        ap.error("--pack goes with --scales")
    if args.gutter and not args.pack:
        ap.error("--gutter goes with --pack")
    if args.gutter < 0:
        ap.error("--gutter must not be negative")
    if args.tiled and args.fit:
        ap.error("--tiled and --fit exclude each other")
    if args.tiled and args.rotate:
        ap.error("--tiled and --rotate exclude each other")
    if args.draw and (args.anonymize or args.chips):
        ap.error("--draw, --anonymize and --chips are separate runs")
    if args.blur is not None and not args.anonymize:
        ap.error("--blur goes with --anonymize")
    if args.anonymize and args.chips:
        ap.error("--anonymize and --chips are separate runs")
    if args.draw:
        dets, _ = annotate_file(args.image, args.draw, label=args.label, tiled=args.tiled, fit=args.fit, flip=args.flip, rotate=args.rotate, scales=args.scales, pack=args.pack, gutter=args.gutter)
    elif args.chips:
        (dets, _), _ = chips_file(args.image, args.chips, size=args.size, tiled=args.tiled, fit=args.fit, flip=args.flip, rotate=args.rotate, scales=args.scales, pack=args.pack, gutter=args.gutter)
    elif args.anonymize and args.blur is not None:
        dets, _ = anonymize_file(args.image, args.anonymize, mode="blur", shape=args.shape, radius=args.blur, scale=args.scale, tiled=args.tiled, fit=args.fit, flip=args.flip, rotate=args.rotate, scales=args.scales, pack=args.pack, gutter=args.gutter)
    elif args.anonymize:
        dets, _ = anonymize_file(args.image, args.anonymize, mode=args.mode, shape=args.shape, cell=args.cell, scale=args.scale, tiled=args.tiled, fit=args.fit, flip=args.flip, rotate=args.rotate, scales=args.scales, pack=args.pack, gutter=args.gutter)
    else:
        from .centerface import CenterFace
        frame = imread(args.image)
        if args.scales:
            detector, frame, views = _views_detector(frame, args.scales, args.tiled, "bf16", args.flip, pack=args.pack, gutter=args.gutter)
            dets, _ = detector.detect_views(frame[None], **views)[0]
        elif args.fit:
            detector = _fit_detector(args.fit, "bf16", args.flip)
            dets, _ = detector.detect_fit(frame[None], rotate=args.rotate)[0]
        elif args.rotate:
            detector = CenterFace(*_upright_hw(frame, args.rotate), dtype="bf16", flip_test=args.flip)
            dets, _ = detector.detect_fit(frame[None], rotate=args.rotate)[0]      # (a context of the upright view's size: the fit fills it)
        else:
            detector = CenterFace(frame.shape[0], frame.shape[1], dtype="bf16", flip_test=args.flip)
            dets, _ = detector(frame)
        detector.close()
    print(format_wider_result(args.image, dets), end="")


if __name__ == "__main__":
    main()

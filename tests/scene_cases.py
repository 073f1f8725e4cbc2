"""The scene check (include/centerface_hip.h "scene cuts", csrc/cf_scene.hip) restated in numpy, line by line, and the frames the tests
run through it.

Integers are Python / int64 integers.  Nothing here knows how the device computes."""
import numpy as np

from follow_cases import FORMATS, canvas, luma_of, planes_of, view  # noqa: F401

FIRST, SAME, CUT = 0, 1, 2
HIST, GRID = 350, 640


def signature(luma):
    """The 128 values of an h x w frame's signature: 64 bins of luma >> 2, then the rounded means of the 8 x 8 cells, row by row."""
    luma = np.asarray(luma).astype(np.int64)
    h, w = luma.shape
    bins = np.bincount((luma >> 2).reshape(-1), minlength=64)[:64]
    mean = np.zeros(64, np.int64)
    for j in range(8):
        for i in range(8):
            cell = luma[(j * h) // 8:((j + 1) * h) // 8, (i * w) // 8:((i + 1) * w) // 8]
            n = cell.size
            mean[8 * j + i] = (int(cell.sum()) + n // 2) // n
    return np.concatenate([bins, mean]).astype(np.int64)


class RefScene(object):
    """The state of a cf_scene: per stream the last signature, the (h, w) it was taken at, valid, run."""

    def __init__(self, streams, hist=HIST, grid=GRID):
        self.hist, self.grid = int(hist), int(grid)
        self.sig = [np.zeros(128, np.int64) for _ in range(streams)]
        self.hw = [(0, 0)] * streams
        self.valid = [False] * streams
        self.run = [0] * streams

    def forget(self, stream=-1):
        for s in range(len(self.valid)) if stream < 0 else [stream]:
            self.valid[s] = False

    def check(self, s, luma):
        """One check of stream s with the frame whose luma is ``luma`` [h, w]: (code, hist, grid, run)."""
        h, w = luma.shape
        sig = signature(luma)
        if not self.valid[s] or self.hw[s] != (h, w):
            code, hist, grid, run = FIRST, 0, 0, 0
        else:
            A = int(np.abs(sig[:64] - self.sig[s][:64]).sum())
            hist = (A * 1000) // (2 * h * w)
            grid = int(np.abs(sig[64:] - self.sig[s][64:]).sum())
            if hist >= self.hist and grid >= self.grid:
                code, run = CUT, 0
            else:
                code, run = SAME, min(self.run[s] + 1, 1 << 30)
        self.sig[s], self.hw[s], self.valid[s], self.run[s] = sig, (h, w), True, run
        return code, hist, grid, run


def run_scene(lumas, streams, hist=HIST, grid=GRID):
    """The tables ``ops.scene_sequence(..., sigs=True)`` returns, from the restatement.  lumas[f * S + s] = the luma of frame f of stream s."""
    S = int(streams)
    F = len(lumas) // S
    ref = RefScene(S, hist, grid)
    out, sigs = np.zeros((F, S, 4), np.int32), np.zeros((F, S, 128), np.int32)
    for f in range(F):
        for s in range(S):
            out[f, s] = ref.check(s, lumas[f * S + s])
            sigs[f, s] = ref.sig[s]
    return out, sigs


# ---------------------------------------------------------------------------------------------- frames
def scene(rng, fmt, h, w, lo, hi, block=4):
    """A block texture with values in [lo, hi), constant over block x block pixels: uint8 [h, w] for 4:2:0, [h, w, 3] for BGR.  The luma
    of a BGR pixel with all three bytes in [lo, hi) is in [lo, hi) too (the weights sum to 256)."""
    shape = ((h + block - 1) // block, (w + block - 1) // block) + ((3,) if fmt == "bgr" else ())
    a = rng.integers(lo, hi, shape, dtype=np.uint8)
    return np.repeat(np.repeat(a, block, axis=0), block, axis=1)[:h, :w]


def moved_views(rng, fmt, h, w, moves, margin=8):
    """Views of one ``follow_cases.canvas`` moved by the (tx, ty) of ``moves``, |tx|, |ty| <= margin."""
    cv = canvas(rng, fmt, h, w, margin)
    return [np.ascontiguousarray(view(cv, h, w, margin, tx, ty)) for tx, ty in moves]


def brighter(img, d):
    """The frame with every byte raised by d, saturating."""
    return np.clip(np.asarray(img).astype(np.int64) + d, 0, 255).astype(np.uint8)


def pack(rng, fmt, imgs, pad0=0, pad1=0):
    """The frames as per-frame tuples of pitched row views whose padding bytes are random (``follow_cases.planes_of``), and their lumas."""
    frames = [planes_of(rng, fmt, im, pad0, pad1) for im in imgs]
    return frames, [luma_of(f, fmt) for f in frames]


def dense(fmt, imgs, rng):
    """The frames as one dense array -- BGR [B,h,w,3], 4:2:0 [B, h*3//2, w] with noise for chroma -- and their lumas."""
    if fmt == "bgr":
        a = np.ascontiguousarray(np.stack(imgs), dtype=np.uint8)
        return a, [luma_of((im.reshape(im.shape[0], -1),), fmt) for im in a]
    h, w = imgs[0].shape
    a = rng.integers(0, 256, (len(imgs), h * 3 // 2, w), dtype=np.uint8)
    for k, im in enumerate(imgs):
        a[k, :h] = im
    return a, [a[k, :h].astype(np.int64) for k in range(len(imgs))]

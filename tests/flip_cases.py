"""The flip test restated in numpy (include/centerface_hip.h under cf_set_flip_test; csrc/cf_flip.hip): the mirror of a network input
batch, the merge of the head records of a batch and its mirrored pass in float32 in the stated order, and the header's worked example.
Shared by tests/test_flip_abi.py (no GPU) and tests/test_flip.py (GPU): the device results must equal these bit for bit."""
import numpy as np

PAIR = (1, 0, 2, 4, 3)          # the point the mirrored pass calls j is the unmirrored pass's PAIR[j] (reference dataset/dataset.py:166-174)
HALF = np.float32(0.5)


def mirror_ref(x, in_format=None):
    """The columns of every image reversed: uint8 [B, H, W, 3] (in_format 0; whole pixels change places, not bytes) or float32
    [B, 3, H, W] (in_format 1).  in_format None: by dtype."""
    x = np.asarray(x)
    if in_format is None:
        in_format = 0 if x.dtype == np.uint8 else 1
    if in_format == 0:
        assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[3] == 3, (x.dtype, x.shape)
        return np.ascontiguousarray(x[:, :, ::-1, :])
    assert in_format == 1 and x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == 3, (in_format, x.dtype, x.shape)
    return np.ascontiguousarray(x[:, :, :, ::-1])


def flip_heads_ref(records_2B, B):
    """records_2B float32 [2B, h, w, 16] -> (records [B, h, w, 16], hm_plane [B, h * w]).  Every value is one float32 addition or
    subtraction and one float32 multiplication by 0.5, in that order."""
    r = np.asarray(records_2B)
    assert r.dtype == np.float32 and r.ndim == 4 and r.shape[0] == 2 * B and r.shape[3] == 16, (r.dtype, r.shape, B)
    a = r[:B]
    m = r[B:, :, ::-1, :]                                   # m[b][y][x] = rec[B + b][y][w - 1 - x]
    out = np.empty_like(a)
    for k in (0, 1, 2, 15):
        out[..., k] = (a[..., k] + m[..., k]) * HALF
    for j, p in enumerate(PAIR):
        out[..., 3 + 2 * j] = (a[..., 3 + 2 * j] - m[..., 3 + 2 * p]) * HALF
        out[..., 4 + 2 * j] = (a[..., 4 + 2 * j] + m[..., 4 + 2 * p]) * HALF
    out[..., 13:15] = a[..., 13:15]
    assert out.dtype == np.float32
    return out, np.ascontiguousarray(out[..., 0]).reshape(B, -1)


def records_to_maps(rec):
    """[B, h, w, 16] records -> the NCHW maps cf_get_heads returns: hm (the logit, r[15]), hm_sigmoid (r[0]), wh, lm, reg."""
    t = np.ascontiguousarray(np.transpose(rec, (0, 3, 1, 2)))
    return {"hm": t[:, 15:16], "hm_sigmoid": t[:, 0:1], "wh": t[:, 1:3], "lm": t[:, 3:13], "reg": t[:, 13:15]}


def maps_to_records(heads):
    """The inverse: the dict of Engine.heads(sigmoid_hm=True) -> [B, h, w, 16] records."""
    t = np.concatenate([heads["hm_sigmoid"], heads["wh"], heads["lm"], heads["reg"], heads["hm"]], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.transpose(t, (0, 2, 3, 1)))


# The header's worked example: B = 1, h = 1, w = 2.  rec[0][0][0] pairs with rec[1][0][1], rec[0][0][1] with rec[1][0][0].
_A0 = (0.75, 4, 6, 1, -2, 3, 0.5, -1, 2.5, 5, -3, 0.25, 8, 0.125, 0.875, 1.5)
_M0 = (0.25, 2, 10, -3, 4, 2, -1, 7, 0.5, 1.5, -5, 3, 6, 0.5, 0.25, -0.5)
_O0 = (0.5, 3, 8, -0.5, -1.5, 3, 2.25, -4, 1.5, 1, 1.5, -0.625, 1.5, 0.125, 0.875, 0.5)
_A1 = (0.5, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.25, 0.75, 0)
_M1 = (0.5, 3, 5, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 9, 9, 2)
_O1 = (0.5, 2, 3, -3, 4, -1, 2, -5, 6, -9, 10, -7, 8, 0.25, 0.75, 1)
WORKED_RECORDS = np.array([[[_A0, _A1]], [[_M1, _M0]]], np.float32)          # [2, 1, 2, 16]
WORKED_OUT = np.array([[[_O0, _O1]]], np.float32)                            # [1, 1, 2, 16]
WORKED_PLANE = np.array([[0.5, 0.5]], np.float32)

"""cf_uphead.hip, bf16: a workgroup of the fused up3+heads kernel walks a RUN of tiles (csrc/cf_uphead.hip: uphead_runs_kernel) --
the next tile's loads are issued under the current tile's head conv, and a tile directly below the previous one takes its two upper
halo rows from LDS instead of fetching and computing them again.  The arithmetic of a pixel is unchanged, so every case here is
BIT-equal to the independent two-kernel path (``uphead=False``: cf_pw.hip's IDAUp epilogue, then cf_head.hip) on seeded random uint8
images, where any stale or mis-addressed halo row changes bits.

The existing test_fused_up3_heads_bit_equal_to_two_kernels runs at batch 3: one tile per workgroup.  The cases here size the batch from
the launcher's rule so that runs of two and three tiles, every kind of run break (next column, next image) and partial tiles occur, and
each asserts the run lengths it expects from that rule: if the rule changes, the case fails instead of silently testing nothing.
"""
import numpy as np
import pytest
import torch

import centerface_amd as cfa

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 16, 32          # uphead_runs_kernel's output tile on the stride-4 map


def _slots():
    """Workgroups of the kernel the device holds at once: two per CU (launch rule in cf_uphead.hip: uphead_slots)."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _tiles(H, W):
    h, w = H // 4, W // 4
    return (w + TILE_W - 1) // TILE_W, (h + TILE_H - 1) // TILE_H


def _runs(T):
    """Run lengths by the launcher's rule: G = min(T, slots) workgroups, workgroup w owns tiles [w T // G, (w + 1) T // G)."""
    G = min(T, _slots())
    return [(w + 1) * T // G - w * T // G for w in range(G)]


def _smallest_batch(H, W, above):
    tx, ty = _tiles(H, W)
    return above // (tx * ty) + 1


def _check(H, W, B, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    ef = cfa.Engine(H, W, max_batch=B, dtype="bf16", uphead=True)
    e2 = cfa.Engine(H, W, max_batch=B, dtype="bf16", uphead=False)
    try:
        assert any(op["name"] == "up3+heads" for op in ef.plan()) and not any(op["name"] == "up3+heads" for op in e2.plan())
        ef.forward_enqueue(x); e2.forward_enqueue(x)
        hf, h2 = ef.heads(sigmoid_hm=True), e2.heads(sigmoid_hm=True)
        for k in ("hm", "wh", "lm", "reg", "hm_sigmoid"):
            assert np.array_equal(hf[k], h2[k]), (k, int((hf[k] != h2[k]).sum()))
        df, d2 = ef.decode_topk(50), e2.decode_topk(50)
        for a, b in zip(df, d2):
            assert np.array_equal(a, b)
    finally:
        ef.close(); e2.close()


def test_long_vertical_runs():
    """640x128 -> a 160x32 map: one tile column of ten tile rows.  With T > 2 slots every workgroup owns two or three tiles; most steps
    go to the tile below (halo rows reused), some runs cross an image boundary (a full halo tile with the zero row above the map)."""
    H, W = 640, 128
    assert _tiles(H, W) == (1, 10)
    B = _smallest_batch(H, W, 2 * _slots())
    runs = _runs(10 * B)
    assert (min(runs), max(runs)) == (2, 3) and sum(runs) == 10 * B
    _check(H, W, B, 1)


def test_every_run_break_and_partial_tiles():
    """160x160 -> a 40x40 map: three tile rows (the last 8 cells high), two tile columns (the second 8 cells wide), six tiles an image.
    Runs of two and three tiles step onto a partial tile with reuse, to the top of the next column and to the next image, where halo
    row -1 must be the zero padding and not the previous tile's rows."""
    H, W = 160, 160
    assert _tiles(H, W) == (2, 3)
    B = _smallest_batch(H, W, 2 * _slots())
    runs = _runs(6 * B)
    assert (min(runs), max(runs)) == (2, 3) and sum(runs) == 6 * B
    _check(H, W, B, 2)


@pytest.mark.parametrize("size,B", [((64, 128), 1), ((128, 128), 1), ((32, 32), 2)])
def test_degenerate_runs(size, B):
    """Exactly one tile; two stacked tiles that are two one-tile workgroups (T <= slots: no CU is lost to runs); an 8x8 map."""
    H, W = size
    tx, ty = _tiles(H, W)
    runs = _runs(tx * ty * B)
    assert (tx, ty) == {(64, 128): (1, 1), (128, 128): (1, 2), (32, 32): (1, 1)}[size]
    assert (min(runs), max(runs)) == (1, 1) and len(runs) == tx * ty * B
    _check(H, W, B, 3 + H)


def test_mixed_runs_at_the_benchmark_size():
    """640x640 at the smallest batch with T > slots: only some workgroups own two tiles, runs of one and two are mixed."""
    H, W = 640, 640
    assert _tiles(H, W) == (5, 10)
    B = _smallest_batch(H, W, _slots())
    runs = _runs(50 * B)
    assert (min(runs), max(runs)) == (1, 2) and sum(runs) == 50 * B
    _check(H, W, B, 4)

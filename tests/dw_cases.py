"""The case table of tests/test_dw_sweep.py, as plain data, and the float64 restatement of the depthwise op it is checked against.

Importable without a GPU: tests/test_dw_cases.py proves that every row lands where it says (``ops.dw_pick``, the host half of the
launcher) and that the table as a whole visits every item of the list below for each of the eleven ``(k, s, TH, TW)`` instances the
release picker of csrc/cf_dw.hip hands out, in both storage types; it also shows that the bounds of the sweep can see the faults this
family is prone to, and ties ``ref64`` to the oracle.

The experiments build is not swept: ``CF_DW_TILE`` / ``CF_DW_CAP`` / ``CF_DW_WGS`` / ``CF_DW2_TILE``, the band and the marching
kernels exist only there (make EXP=1); the release library contains none of those paths and reads none of those variables.

A case = (id, dtype, C, H, W, k, stride, pad, act, bias, B, instance, Cc, nchunk, threads).  ``pad``: "same" = the reference's rule
(k - stride zeros in all, the smaller half in front: asymmetric at stride 2), "sym" = the ShuffleV2 block's k // 2 on both sides.
``instance`` = "strip<k,s,TH,TW>" (dw_strip_kernel) or "lds<k,s,TH,TW>" (dw_lds_kernel); ``full_tag`` makes the symbol
``ops.last_kernel()`` must report from it.  (Cc, nchunk, threads) = channels per chunk, chunks, threads per workgroup.

Ids: <instance letter><f | b = fp32 | bf16>-<what>.  Instances (INSTANCES below): A B C = 3x3 stride 1 on 16x32 / 8x40 / 10x20,
D E F = 5x5 stride 1 on 16x16 / 20x20 / 10x20, G H I = 3x3 stride 2 on 10x20 / 4x32 / 4x16, J K = 5x5 stride 2 on 8x16 / 4x32.
What (output sizes; T = the tile, w0 = the first width of a class that starts above one tile):
  row    one output row (G: nine, its class starts there), T_w - 1 or w0 wide; C = 8: one 16-byte group per pixel in bf16, two in fp32
  t1     one row and one column more than a tile (more than w0): four tiles in the small classes; C = 16; odd stride-2 inputs
  tm     a tile - 1 (w0 wide in the wide classes); C = 24
  c32    C = 32, two rows, B = 3
  r1-3   Wo % 4 = 1, 2, 3: strips cut by the right edge (strip kernels)
  1x1    a 1 x 1 input (the classes that hold Wo = 1; stride 2 under the symmetric pad only: the reference's rule leaves no window)
  edge   C = two chunks of the LARGEST channel chunk the instance's LDS budget holds (tests/test_dw_cases.py proves that one more
         16-byte group does not fit)
  prime  C = 8 x 37: no divisor but 8 channels fits, 37 chunks; B = 3 and an odd number of tiles: an odd work list
  e0-3   stride 2: act x bias = swish / none x without / with -- the four template instances of dw_lds_kernel on the tile
  few    a work list shorter than 8 workgroups (B = 1 where two images already make 8; A's class starts at 8 tiles per row)
X<f|b>-... = both sides of every class boundary of the picker.
"""
import numpy as np

CASES = (
    ('Af-row', 'fp32', 8, 1, 256, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 8, 1, 256),
    ('Af-t1', 'fp32', 16, 17, 257, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,16,32>', 16, 1, 256),
    ('Af-tm', 'fp32', 24, 15, 256, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 24, 1, 256),
    ('Af-c32', 'fp32', 32, 2, 257, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,16,32>', 16, 2, 256),
    ('Af-r1', 'fp32', 8, 3, 257, 3, 1, 'same', 'none', True, 2, 'strip<3,1,16,32>', 8, 1, 256),
    ('Af-r2', 'fp32', 16, 3, 258, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 16, 1, 256),
    ('Af-r3', 'fp32', 24, 3, 259, 3, 1, 'same', 'none', True, 2, 'strip<3,1,16,32>', 24, 1, 256),
    ('Af-edge', 'fp32', 48, 5, 257, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 24, 2, 256),
    ('Af-prime', 'fp32', 296, 2, 257, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,16,32>', 8, 37, 256),
    ('Ab-row', 'bf16', 8, 1, 256, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 8, 1, 128),
    ('Ab-t1', 'bf16', 16, 17, 257, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,16,32>', 16, 1, 256),
    ('Ab-tm', 'bf16', 24, 15, 256, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 24, 1, 256),
    ('Ab-c32', 'bf16', 32, 2, 257, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,16,32>', 32, 1, 256),
    ('Ab-r1', 'bf16', 8, 3, 257, 3, 1, 'same', 'none', True, 2, 'strip<3,1,16,32>', 8, 1, 128),
    ('Ab-r2', 'bf16', 16, 3, 258, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 16, 1, 256),
    ('Ab-r3', 'bf16', 24, 3, 259, 3, 1, 'same', 'none', True, 2, 'strip<3,1,16,32>', 24, 1, 256),
    ('Ab-edge', 'bf16', 96, 5, 257, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 48, 2, 256),
    ('Ab-prime', 'bf16', 296, 2, 257, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,16,32>', 8, 37, 128),
    ('Bf-row', 'fp32', 8, 1, 96, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 8, 1, 192),
    ('Bf-t1', 'fp32', 16, 9, 97, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,8,40>', 16, 1, 256),
    ('Bf-tm', 'fp32', 24, 7, 96, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 24, 1, 256),
    ('Bf-c32', 'fp32', 32, 2, 97, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,8,40>', 16, 2, 256),
    ('Bf-r1', 'fp32', 8, 3, 97, 3, 1, 'same', 'none', True, 2, 'strip<3,1,8,40>', 8, 1, 192),
    ('Bf-r2', 'fp32', 16, 3, 98, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 16, 1, 256),
    ('Bf-r3', 'fp32', 24, 3, 99, 3, 1, 'same', 'none', True, 2, 'strip<3,1,8,40>', 24, 1, 256),
    ('Bf-edge', 'fp32', 56, 5, 97, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 28, 2, 256),
    ('Bf-prime', 'fp32', 296, 2, 97, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,8,40>', 8, 37, 192),
    ('Bf-few', 'fp32', 8, 1, 96, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,8,40>', 8, 1, 192),
    ('Bb-row', 'bf16', 8, 1, 96, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 8, 1, 128),
    ('Bb-t1', 'bf16', 16, 9, 97, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,8,40>', 16, 1, 192),
    ('Bb-tm', 'bf16', 24, 7, 96, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 24, 1, 256),
    ('Bb-c32', 'bf16', 32, 2, 97, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,8,40>', 32, 1, 256),
    ('Bb-r1', 'bf16', 8, 3, 97, 3, 1, 'same', 'none', True, 2, 'strip<3,1,8,40>', 8, 1, 128),
    ('Bb-r2', 'bf16', 16, 3, 98, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 16, 1, 192),
    ('Bb-r3', 'bf16', 24, 3, 99, 3, 1, 'same', 'none', True, 2, 'strip<3,1,8,40>', 24, 1, 256),
    ('Bb-edge', 'bf16', 112, 5, 97, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 56, 2, 256),
    ('Bb-prime', 'bf16', 296, 2, 97, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,8,40>', 8, 37, 128),
    ('Bb-few', 'bf16', 8, 1, 96, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,8,40>', 8, 1, 128),
    ('Cf-row', 'fp32', 8, 1, 19, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 8, 1, 128),
    ('Cf-t1', 'fp32', 16, 11, 21, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,10,20>', 16, 1, 256),
    ('Cf-tm', 'fp32', 24, 9, 19, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 24, 1, 256),
    ('Cf-c32', 'fp32', 32, 2, 21, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,10,20>', 32, 1, 256),
    ('Cf-r1', 'fp32', 8, 3, 17, 3, 1, 'same', 'none', True, 2, 'strip<3,1,10,20>', 8, 1, 128),
    ('Cf-r2', 'fp32', 16, 3, 18, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 16, 1, 256),
    ('Cf-r3', 'fp32', 24, 3, 19, 3, 1, 'same', 'none', True, 2, 'strip<3,1,10,20>', 24, 1, 256),
    ('Cf-1x1', 'fp32', 16, 1, 1, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,10,20>', 16, 1, 256),
    ('Cf-edge', 'fp32', 88, 5, 21, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 44, 2, 256),
    ('Cf-prime', 'fp32', 296, 2, 19, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,10,20>', 8, 37, 128),
    ('Cf-few', 'fp32', 8, 1, 19, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,10,20>', 8, 1, 128),
    ('Cb-row', 'bf16', 8, 1, 19, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 8, 1, 64),
    ('Cb-t1', 'bf16', 16, 11, 21, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,10,20>', 16, 1, 128),
    ('Cb-tm', 'bf16', 24, 9, 19, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 24, 1, 192),
    ('Cb-c32', 'bf16', 32, 2, 21, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,10,20>', 32, 1, 256),
    ('Cb-r1', 'bf16', 8, 3, 17, 3, 1, 'same', 'none', True, 2, 'strip<3,1,10,20>', 8, 1, 64),
    ('Cb-r2', 'bf16', 16, 3, 18, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 16, 1, 128),
    ('Cb-r3', 'bf16', 24, 3, 19, 3, 1, 'same', 'none', True, 2, 'strip<3,1,10,20>', 24, 1, 192),
    ('Cb-1x1', 'bf16', 16, 1, 1, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,10,20>', 16, 1, 128),
    ('Cb-edge', 'bf16', 160, 5, 21, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 80, 2, 256),
    ('Cb-prime', 'bf16', 296, 2, 19, 3, 1, 'sym', 'none', True, 3, 'strip<3,1,10,20>', 8, 37, 64),
    ('Cb-few', 'bf16', 8, 1, 19, 3, 1, 'sym', 'none', True, 2, 'strip<3,1,10,20>', 8, 1, 64),
    ('Df-row', 'fp32', 8, 1, 64, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 8, 1, 128),
    ('Df-t1', 'fp32', 16, 17, 65, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,16,16>', 16, 1, 256),
    ('Df-tm', 'fp32', 24, 15, 64, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 12, 2, 192),
    ('Df-c32', 'fp32', 32, 2, 65, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,16,16>', 16, 2, 256),
    ('Df-r1', 'fp32', 8, 3, 65, 5, 1, 'same', 'none', True, 2, 'strip<5,1,16,16>', 8, 1, 128),
    ('Df-r2', 'fp32', 16, 3, 66, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 16, 1, 256),
    ('Df-r3', 'fp32', 24, 3, 67, 5, 1, 'same', 'none', True, 2, 'strip<5,1,16,16>', 12, 2, 192),
    ('Df-edge', 'fp32', 32, 5, 65, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 16, 2, 256),
    ('Df-prime', 'fp32', 296, 2, 65, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,16,16>', 8, 37, 128),
    ('Df-few', 'fp32', 8, 1, 64, 5, 1, 'sym', 'none', True, 1, 'strip<5,1,16,16>', 8, 1, 128),
    ('Db-row', 'bf16', 8, 1, 64, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 8, 1, 64),
    ('Db-t1', 'bf16', 16, 17, 65, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,16,16>', 16, 1, 128),
    ('Db-tm', 'bf16', 24, 15, 64, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 24, 1, 192),
    ('Db-c32', 'bf16', 32, 2, 65, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,16,16>', 32, 1, 256),
    ('Db-r1', 'bf16', 8, 3, 65, 5, 1, 'same', 'none', True, 2, 'strip<5,1,16,16>', 8, 1, 64),
    ('Db-r2', 'bf16', 16, 3, 66, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 16, 1, 128),
    ('Db-r3', 'bf16', 24, 3, 67, 5, 1, 'same', 'none', True, 2, 'strip<5,1,16,16>', 24, 1, 192),
    ('Db-edge', 'bf16', 64, 5, 65, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 32, 2, 256),
    ('Db-prime', 'bf16', 296, 2, 65, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,16,16>', 8, 37, 64),
    ('Db-few', 'bf16', 8, 1, 64, 5, 1, 'sym', 'none', True, 1, 'strip<5,1,16,16>', 8, 1, 64),
    ('Ef-row', 'fp32', 8, 1, 32, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 8, 1, 256),
    ('Ef-t1', 'fp32', 16, 21, 33, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Ef-tm', 'fp32', 24, 19, 32, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 12, 2, 256),
    ('Ef-c32', 'fp32', 32, 2, 33, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,20,20>', 16, 2, 256),
    ('Ef-r1', 'fp32', 8, 3, 33, 5, 1, 'same', 'none', True, 2, 'strip<5,1,20,20>', 8, 1, 256),
    ('Ef-r2', 'fp32', 16, 3, 34, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Ef-r3', 'fp32', 24, 3, 35, 5, 1, 'same', 'none', True, 2, 'strip<5,1,20,20>', 12, 2, 256),
    ('Ef-edge', 'fp32', 40, 5, 33, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 20, 2, 256),
    ('Ef-prime', 'fp32', 296, 2, 43, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,20,20>', 8, 37, 256),
    ('Ef-few', 'fp32', 8, 1, 32, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,20,20>', 8, 1, 256),
    ('Eb-row', 'bf16', 8, 1, 32, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 8, 1, 128),
    ('Eb-t1', 'bf16', 16, 21, 33, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Eb-tm', 'bf16', 24, 19, 32, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 24, 1, 256),
    ('Eb-c32', 'bf16', 32, 2, 33, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,20,20>', 32, 1, 256),
    ('Eb-r1', 'bf16', 8, 3, 33, 5, 1, 'same', 'none', True, 2, 'strip<5,1,20,20>', 8, 1, 128),
    ('Eb-r2', 'bf16', 16, 3, 34, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Eb-r3', 'bf16', 24, 3, 35, 5, 1, 'same', 'none', True, 2, 'strip<5,1,20,20>', 24, 1, 256),
    ('Eb-edge', 'bf16', 64, 5, 33, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 32, 2, 256),
    ('Eb-prime', 'bf16', 296, 2, 43, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,20,20>', 8, 37, 128),
    ('Eb-few', 'bf16', 8, 1, 32, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,20,20>', 8, 1, 128),
    ('Ff-row', 'fp32', 8, 1, 19, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 8, 1, 128),
    ('Ff-t1', 'fp32', 16, 11, 21, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,10,20>', 16, 1, 256),
    ('Ff-tm', 'fp32', 24, 9, 19, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 12, 2, 192),
    ('Ff-c32', 'fp32', 32, 2, 21, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,10,20>', 16, 2, 256),
    ('Ff-r1', 'fp32', 8, 3, 17, 5, 1, 'same', 'none', True, 2, 'strip<5,1,10,20>', 8, 1, 128),
    ('Ff-r2', 'fp32', 16, 3, 18, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 16, 1, 256),
    ('Ff-r3', 'fp32', 24, 3, 19, 5, 1, 'same', 'none', True, 2, 'strip<5,1,10,20>', 12, 2, 192),
    ('Ff-1x1', 'fp32', 16, 1, 1, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,10,20>', 16, 1, 256),
    ('Ff-edge', 'fp32', 40, 5, 21, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 20, 2, 256),
    ('Ff-prime', 'fp32', 296, 2, 19, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,10,20>', 8, 37, 128),
    ('Ff-few', 'fp32', 8, 1, 19, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,10,20>', 8, 1, 128),
    ('Fb-row', 'bf16', 8, 1, 19, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 8, 1, 64),
    ('Fb-t1', 'bf16', 16, 11, 21, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,10,20>', 16, 1, 128),
    ('Fb-tm', 'bf16', 24, 9, 19, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 24, 1, 192),
    ('Fb-c32', 'bf16', 32, 2, 21, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,10,20>', 32, 1, 256),
    ('Fb-r1', 'bf16', 8, 3, 17, 5, 1, 'same', 'none', True, 2, 'strip<5,1,10,20>', 8, 1, 64),
    ('Fb-r2', 'bf16', 16, 3, 18, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 16, 1, 128),
    ('Fb-r3', 'bf16', 24, 3, 19, 5, 1, 'same', 'none', True, 2, 'strip<5,1,10,20>', 24, 1, 192),
    ('Fb-1x1', 'bf16', 16, 1, 1, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,10,20>', 16, 1, 128),
    ('Fb-edge', 'bf16', 80, 5, 21, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 40, 2, 256),
    ('Fb-prime', 'bf16', 296, 2, 19, 5, 1, 'sym', 'none', True, 3, 'strip<5,1,10,20>', 8, 37, 64),
    ('Fb-few', 'bf16', 8, 1, 19, 5, 1, 'sym', 'none', True, 2, 'strip<5,1,10,20>', 8, 1, 64),
    ('Gf-row', 'fp32', 8, 18, 38, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,10,20>', 8, 1, 256),
    ('Gf-t1', 'fp32', 16, 21, 40, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,10,20>', 8, 2, 256),
    ('Gf-tm', 'fp32', 24, 19, 39, 3, 2, 'same', 'swish', True, 2, 'lds<3,2,10,20>', 12, 2, 256),
    ('Gf-c32', 'fp32', 32, 20, 39, 3, 2, 'sym', 'none', False, 3, 'lds<3,2,10,20>', 8, 4, 256),
    ('Gf-edge', 'fp32', 24, 18, 40, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,10,20>', 12, 2, 256),
    ('Gf-prime', 'fp32', 296, 18, 38, 3, 2, 'sym', 'none', True, 3, 'lds<3,2,10,20>', 8, 37, 256),
    ('Gf-e0', 'fp32', 8, 22, 40, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,10,20>', 8, 1, 256),
    ('Gf-e1', 'fp32', 16, 23, 38, 3, 2, 'same', 'none', True, 2, 'lds<3,2,10,20>', 8, 2, 256),
    ('Gf-e2', 'fp32', 24, 22, 39, 3, 2, 'sym', 'swish', True, 2, 'lds<3,2,10,20>', 12, 2, 256),
    ('Gf-e3', 'fp32', 32, 21, 37, 3, 2, 'sym', 'none', False, 2, 'lds<3,2,10,20>', 8, 4, 256),
    ('Gf-few', 'fp32', 8, 18, 38, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,10,20>', 8, 1, 256),
    ('Gb-row', 'bf16', 8, 18, 38, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,10,20>', 8, 1, 256),
    ('Gb-t1', 'bf16', 16, 21, 40, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,10,20>', 16, 1, 256),
    ('Gb-tm', 'bf16', 24, 19, 39, 3, 2, 'same', 'swish', True, 2, 'lds<3,2,10,20>', 24, 1, 256),
    ('Gb-c32', 'bf16', 32, 20, 39, 3, 2, 'sym', 'none', False, 3, 'lds<3,2,10,20>', 16, 2, 256),
    ('Gb-edge', 'bf16', 48, 18, 40, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,10,20>', 24, 2, 256),
    ('Gb-prime', 'bf16', 296, 18, 38, 3, 2, 'sym', 'none', True, 3, 'lds<3,2,10,20>', 8, 37, 256),
    ('Gb-e0', 'bf16', 8, 22, 40, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,10,20>', 8, 1, 256),
    ('Gb-e1', 'bf16', 16, 23, 38, 3, 2, 'same', 'none', True, 2, 'lds<3,2,10,20>', 16, 1, 256),
    ('Gb-e2', 'bf16', 24, 22, 39, 3, 2, 'sym', 'swish', True, 2, 'lds<3,2,10,20>', 24, 1, 256),
    ('Gb-e3', 'bf16', 32, 21, 37, 3, 2, 'sym', 'none', False, 2, 'lds<3,2,10,20>', 16, 2, 256),
    ('Gb-few', 'bf16', 8, 18, 38, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,10,20>', 8, 1, 256),
    ('Hf-row', 'fp32', 8, 2, 128, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 8, 1, 256),
    ('Hf-t1', 'fp32', 16, 9, 130, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,32>', 16, 1, 256),
    ('Hf-tm', 'fp32', 24, 7, 129, 3, 2, 'same', 'swish', True, 2, 'lds<3,2,4,32>', 12, 2, 256),
    ('Hf-c32', 'fp32', 32, 4, 129, 3, 2, 'sym', 'none', False, 3, 'lds<3,2,4,32>', 16, 2, 256),
    ('Hf-edge', 'fp32', 40, 10, 130, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 20, 2, 256),
    ('Hf-prime', 'fp32', 296, 4, 130, 3, 2, 'sym', 'none', True, 3, 'lds<3,2,4,32>', 8, 37, 256),
    ('Hf-e0', 'fp32', 8, 6, 130, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 8, 1, 256),
    ('Hf-e1', 'fp32', 16, 7, 128, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,32>', 16, 1, 256),
    ('Hf-e2', 'fp32', 24, 6, 129, 3, 2, 'sym', 'swish', True, 2, 'lds<3,2,4,32>', 12, 2, 256),
    ('Hf-e3', 'fp32', 32, 5, 127, 3, 2, 'sym', 'none', False, 2, 'lds<3,2,4,32>', 16, 2, 256),
    ('Hf-few', 'fp32', 8, 2, 128, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,32>', 8, 1, 256),
    ('Hb-row', 'bf16', 8, 2, 128, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 8, 1, 256),
    ('Hb-t1', 'bf16', 16, 9, 130, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,32>', 16, 1, 256),
    ('Hb-tm', 'bf16', 24, 7, 129, 3, 2, 'same', 'swish', True, 2, 'lds<3,2,4,32>', 24, 1, 256),
    ('Hb-c32', 'bf16', 32, 4, 129, 3, 2, 'sym', 'none', False, 3, 'lds<3,2,4,32>', 32, 1, 256),
    ('Hb-edge', 'bf16', 80, 10, 130, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 40, 2, 256),
    ('Hb-prime', 'bf16', 296, 4, 130, 3, 2, 'sym', 'none', True, 3, 'lds<3,2,4,32>', 8, 37, 256),
    ('Hb-e0', 'bf16', 8, 6, 130, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 8, 1, 256),
    ('Hb-e1', 'bf16', 16, 7, 128, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,32>', 16, 1, 256),
    ('Hb-e2', 'bf16', 24, 6, 129, 3, 2, 'sym', 'swish', True, 2, 'lds<3,2,4,32>', 24, 1, 256),
    ('Hb-e3', 'bf16', 32, 5, 127, 3, 2, 'sym', 'none', False, 2, 'lds<3,2,4,32>', 32, 1, 256),
    ('Hb-few', 'bf16', 8, 2, 128, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,32>', 8, 1, 256),
    ('If-row', 'fp32', 8, 2, 30, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 8, 1, 256),
    ('If-t1', 'fp32', 16, 9, 34, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('If-tm', 'fp32', 24, 7, 31, 3, 2, 'same', 'swish', True, 2, 'lds<3,2,4,16>', 12, 2, 256),
    ('If-c32', 'fp32', 32, 4, 33, 3, 2, 'sym', 'none', False, 3, 'lds<3,2,4,16>', 16, 2, 256),
    ('If-1x1', 'fp32', 16, 1, 1, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('If-edge', 'fp32', 40, 10, 34, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 20, 2, 256),
    ('If-prime', 'fp32', 296, 4, 30, 3, 2, 'sym', 'none', True, 3, 'lds<3,2,4,16>', 8, 37, 256),
    ('If-e0', 'fp32', 8, 6, 34, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 8, 1, 256),
    ('If-e1', 'fp32', 16, 7, 32, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('If-e2', 'fp32', 24, 6, 33, 3, 2, 'sym', 'swish', True, 2, 'lds<3,2,4,16>', 12, 2, 256),
    ('If-e3', 'fp32', 32, 5, 31, 3, 2, 'sym', 'none', False, 2, 'lds<3,2,4,16>', 16, 2, 256),
    ('If-few', 'fp32', 8, 2, 30, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,16>', 8, 1, 256),
    ('Ib-row', 'bf16', 8, 2, 30, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 8, 1, 256),
    ('Ib-t1', 'bf16', 16, 9, 34, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('Ib-tm', 'bf16', 24, 7, 31, 3, 2, 'same', 'swish', True, 2, 'lds<3,2,4,16>', 24, 1, 256),
    ('Ib-c32', 'bf16', 32, 4, 33, 3, 2, 'sym', 'none', False, 3, 'lds<3,2,4,16>', 32, 1, 256),
    ('Ib-1x1', 'bf16', 16, 1, 1, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('Ib-edge', 'bf16', 80, 10, 34, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 40, 2, 256),
    ('Ib-prime', 'bf16', 296, 4, 30, 3, 2, 'sym', 'none', True, 3, 'lds<3,2,4,16>', 8, 37, 256),
    ('Ib-e0', 'bf16', 8, 6, 34, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 8, 1, 256),
    ('Ib-e1', 'bf16', 16, 7, 32, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('Ib-e2', 'bf16', 24, 6, 33, 3, 2, 'sym', 'swish', True, 2, 'lds<3,2,4,16>', 24, 1, 256),
    ('Ib-e3', 'bf16', 32, 5, 31, 3, 2, 'sym', 'none', False, 2, 'lds<3,2,4,16>', 32, 1, 256),
    ('Ib-few', 'bf16', 8, 2, 30, 3, 2, 'sym', 'none', True, 2, 'lds<3,2,4,16>', 8, 1, 256),
    ('Jf-row', 'fp32', 8, 2, 128, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 8, 1, 256),
    ('Jf-t1', 'fp32', 16, 17, 130, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,8,16>', 8, 2, 256),
    ('Jf-tm', 'fp32', 24, 15, 129, 5, 2, 'same', 'swish', True, 2, 'lds<5,2,8,16>', 8, 3, 256),
    ('Jf-c32', 'fp32', 32, 4, 129, 5, 2, 'sym', 'none', False, 3, 'lds<5,2,8,16>', 8, 4, 256),
    ('Jf-edge', 'fp32', 16, 10, 130, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 8, 2, 256),
    ('Jf-prime', 'fp32', 296, 4, 130, 5, 2, 'sym', 'none', True, 3, 'lds<5,2,8,16>', 8, 37, 256),
    ('Jf-e0', 'fp32', 8, 6, 130, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 8, 1, 256),
    ('Jf-e1', 'fp32', 16, 7, 128, 5, 2, 'same', 'none', True, 2, 'lds<5,2,8,16>', 8, 2, 256),
    ('Jf-e2', 'fp32', 24, 6, 129, 5, 2, 'sym', 'swish', True, 2, 'lds<5,2,8,16>', 8, 3, 256),
    ('Jf-e3', 'fp32', 32, 5, 127, 5, 2, 'sym', 'none', False, 2, 'lds<5,2,8,16>', 8, 4, 256),
    ('Jf-few', 'fp32', 8, 2, 128, 5, 2, 'sym', 'none', True, 1, 'lds<5,2,8,16>', 8, 1, 256),
    ('Jb-row', 'bf16', 8, 2, 128, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 8, 1, 256),
    ('Jb-t1', 'bf16', 16, 17, 130, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,8,16>', 16, 1, 256),
    ('Jb-tm', 'bf16', 24, 15, 129, 5, 2, 'same', 'swish', True, 2, 'lds<5,2,8,16>', 8, 3, 256),
    ('Jb-c32', 'bf16', 32, 4, 129, 5, 2, 'sym', 'none', False, 3, 'lds<5,2,8,16>', 16, 2, 256),
    ('Jb-edge', 'bf16', 32, 10, 130, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 16, 2, 256),
    ('Jb-prime', 'bf16', 296, 4, 130, 5, 2, 'sym', 'none', True, 3, 'lds<5,2,8,16>', 8, 37, 256),
    ('Jb-e0', 'bf16', 8, 6, 130, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 8, 1, 256),
    ('Jb-e1', 'bf16', 16, 7, 128, 5, 2, 'same', 'none', True, 2, 'lds<5,2,8,16>', 16, 1, 256),
    ('Jb-e2', 'bf16', 24, 6, 129, 5, 2, 'sym', 'swish', True, 2, 'lds<5,2,8,16>', 8, 3, 256),
    ('Jb-e3', 'bf16', 32, 5, 127, 5, 2, 'sym', 'none', False, 2, 'lds<5,2,8,16>', 16, 2, 256),
    ('Jb-few', 'bf16', 8, 2, 128, 5, 2, 'sym', 'none', True, 1, 'lds<5,2,8,16>', 8, 1, 256),
    ('Kf-row', 'fp32', 8, 2, 62, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 8, 1, 256),
    ('Kf-t1', 'fp32', 16, 9, 66, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,4,32>', 8, 2, 256),
    ('Kf-tm', 'fp32', 24, 7, 63, 5, 2, 'same', 'swish', True, 2, 'lds<5,2,4,32>', 8, 3, 256),
    ('Kf-c32', 'fp32', 32, 4, 65, 5, 2, 'sym', 'none', False, 3, 'lds<5,2,4,32>', 8, 4, 256),
    ('Kf-1x1', 'fp32', 16, 1, 1, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,4,32>', 8, 2, 256),
    ('Kf-edge', 'fp32', 16, 10, 66, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 8, 2, 256),
    ('Kf-prime', 'fp32', 296, 4, 62, 5, 2, 'sym', 'none', True, 3, 'lds<5,2,4,32>', 8, 37, 256),
    ('Kf-e0', 'fp32', 8, 6, 66, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 8, 1, 256),
    ('Kf-e1', 'fp32', 16, 7, 64, 5, 2, 'same', 'none', True, 2, 'lds<5,2,4,32>', 8, 2, 256),
    ('Kf-e2', 'fp32', 24, 6, 65, 5, 2, 'sym', 'swish', True, 2, 'lds<5,2,4,32>', 8, 3, 256),
    ('Kf-e3', 'fp32', 32, 5, 63, 5, 2, 'sym', 'none', False, 2, 'lds<5,2,4,32>', 8, 4, 256),
    ('Kf-few', 'fp32', 8, 2, 62, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,4,32>', 8, 1, 256),
    ('Kb-row', 'bf16', 8, 2, 62, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 8, 1, 256),
    ('Kb-t1', 'bf16', 16, 9, 66, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,4,32>', 16, 1, 256),
    ('Kb-tm', 'bf16', 24, 7, 63, 5, 2, 'same', 'swish', True, 2, 'lds<5,2,4,32>', 8, 3, 256),
    ('Kb-c32', 'bf16', 32, 4, 65, 5, 2, 'sym', 'none', False, 3, 'lds<5,2,4,32>', 16, 2, 256),
    ('Kb-1x1', 'bf16', 16, 1, 1, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,4,32>', 16, 1, 256),
    ('Kb-edge', 'bf16', 32, 10, 66, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 16, 2, 256),
    ('Kb-prime', 'bf16', 296, 4, 62, 5, 2, 'sym', 'none', True, 3, 'lds<5,2,4,32>', 8, 37, 256),
    ('Kb-e0', 'bf16', 8, 6, 66, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 8, 1, 256),
    ('Kb-e1', 'bf16', 16, 7, 64, 5, 2, 'same', 'none', True, 2, 'lds<5,2,4,32>', 16, 1, 256),
    ('Kb-e2', 'bf16', 24, 6, 65, 5, 2, 'sym', 'swish', True, 2, 'lds<5,2,4,32>', 8, 3, 256),
    ('Kb-e3', 'bf16', 32, 5, 63, 5, 2, 'sym', 'none', False, 2, 'lds<5,2,4,32>', 16, 2, 256),
    ('Kb-few', 'bf16', 8, 2, 62, 5, 2, 'sym', 'none', True, 2, 'lds<5,2,4,32>', 8, 1, 256),
    ('Xf-k3s1-w95', 'fp32', 16, 3, 95, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 16, 1, 256),
    ('Xf-k3s1-w96', 'fp32', 16, 3, 96, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 16, 1, 256),
    ('Xf-k3s1-w255', 'fp32', 16, 3, 255, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 16, 1, 256),
    ('Xf-k3s1-w256', 'fp32', 16, 3, 256, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 16, 1, 256),
    ('Xf-k5s1-w31', 'fp32', 16, 3, 31, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 16, 1, 256),
    ('Xf-k5s1-w32', 'fp32', 16, 3, 32, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Xf-k5s1-w63', 'fp32', 16, 3, 63, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Xf-k5s1-w64', 'fp32', 16, 3, 64, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 16, 1, 256),
    ('Xf-k3s2-w63', 'fp32', 16, 7, 127, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('Xf-k3s2-w64', 'fp32', 16, 6, 128, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 16, 1, 256),
    ('Xf-k5s2-w63', 'fp32', 16, 7, 127, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 8, 2, 256),
    ('Xf-k5s2-w64', 'fp32', 16, 6, 128, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 8, 2, 256),
    ('Xf-k3s2-8x20', 'fp32', 24, 16, 41, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 12, 2, 256),
    ('Xf-k3s2-9x20', 'fp32', 24, 19, 40, 3, 2, 'same', 'none', True, 2, 'lds<3,2,10,20>', 12, 2, 256),
    ('Xf-k3s2-20x20', 'fp32', 24, 40, 41, 3, 2, 'same', 'none', True, 2, 'lds<3,2,10,20>', 12, 2, 256),
    ('Xf-k3s2-21x20', 'fp32', 24, 43, 40, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 12, 2, 256),
    ('Xf-k3s2-20x21', 'fp32', 24, 40, 43, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 12, 2, 256),
    ('Xb-k3s1-w95', 'bf16', 16, 3, 95, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,10,20>', 16, 1, 128),
    ('Xb-k3s1-w96', 'bf16', 16, 3, 96, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 16, 1, 192),
    ('Xb-k3s1-w255', 'bf16', 16, 3, 255, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,8,40>', 16, 1, 192),
    ('Xb-k3s1-w256', 'bf16', 16, 3, 256, 3, 1, 'same', 'swish', False, 2, 'strip<3,1,16,32>', 16, 1, 256),
    ('Xb-k5s1-w31', 'bf16', 16, 3, 31, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,10,20>', 16, 1, 128),
    ('Xb-k5s1-w32', 'bf16', 16, 3, 32, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Xb-k5s1-w63', 'bf16', 16, 3, 63, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,20,20>', 16, 1, 256),
    ('Xb-k5s1-w64', 'bf16', 16, 3, 64, 5, 1, 'same', 'swish', False, 2, 'strip<5,1,16,16>', 16, 1, 128),
    ('Xb-k3s2-w63', 'bf16', 16, 7, 127, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,16>', 16, 1, 256),
    ('Xb-k3s2-w64', 'bf16', 16, 6, 128, 3, 2, 'same', 'swish', False, 2, 'lds<3,2,4,32>', 16, 1, 256),
    ('Xb-k5s2-w63', 'bf16', 16, 7, 127, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,4,32>', 16, 1, 256),
    ('Xb-k5s2-w64', 'bf16', 16, 6, 128, 5, 2, 'same', 'swish', False, 2, 'lds<5,2,8,16>', 16, 1, 256),
    ('Xb-k3s2-8x20', 'bf16', 24, 16, 41, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 24, 1, 256),
    ('Xb-k3s2-9x20', 'bf16', 24, 19, 40, 3, 2, 'same', 'none', True, 2, 'lds<3,2,10,20>', 24, 1, 256),
    ('Xb-k3s2-20x20', 'bf16', 24, 40, 41, 3, 2, 'same', 'none', True, 2, 'lds<3,2,10,20>', 24, 1, 256),
    ('Xb-k3s2-21x20', 'bf16', 24, 43, 40, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 24, 1, 256),
    ('Xb-k3s2-20x21', 'bf16', 24, 40, 43, 3, 2, 'same', 'none', True, 2, 'lds<3,2,4,16>', 24, 1, 256),
)

IDS = tuple(c[0] for c in CASES)
DTYPES = ("fp32", "bf16")
_T = {"bf16": "unsigned short", "fp32": "float", "fp32_split": "float"}      # fp32_split: fp32 storage, and no GEMM in this op

# The eleven instances of the release picker (dw_strip_table / dw_plan in csrc/cf_dw.hip): letter -> (instance, LDS budget in
# KiB, the class of output maps it serves as a predicate on (Ho, Wo)).
INSTANCES = {
    "A": ("strip<3,1,16,32>", 60, lambda ho, wo: wo >= 256),
    "B": ("strip<3,1,8,40>", 48, lambda ho, wo: 96 <= wo < 256),
    "C": ("strip<3,1,10,20>", 48, lambda ho, wo: wo < 96),
    "D": ("strip<5,1,16,16>", 32, lambda ho, wo: wo >= 64),
    "E": ("strip<5,1,20,20>", 48, lambda ho, wo: 32 <= wo < 64),
    "F": ("strip<5,1,10,20>", 32, lambda ho, wo: wo < 32),
    "G": ("lds<3,2,10,20>", 48, lambda ho, wo: 8 < ho <= 20 and wo <= 20),
    "H": ("lds<3,2,4,32>", 48, lambda ho, wo: wo >= 64 and not (8 < ho <= 20 and wo <= 20)),
    "I": ("lds<3,2,4,16>", 24, lambda ho, wo: wo < 64 and not (8 < ho <= 20 and wo <= 20)),
    "J": ("lds<5,2,8,16>", 24, lambda ho, wo: wo >= 64),
    "K": ("lds<5,2,4,32>", 32, lambda ho, wo: wo < 64),
}
# one fp32 case per instance that also runs as "fp32_split" (the same float kernel: bit-equal results)
SPLIT_CASES = tuple(letter + "f-t1" for letter in INSTANCES)

# what cf_op_dwconv refuses before any GPU work (the output stays untouched): (dtype, C, H, W, k, stride, (pad_lo, pad_hi))
REFUSED = {
    "C % 8": ("fp32", 12, 9, 9, 3, 1, (1, 1)),
    "C % 8 (bf16)": ("bf16", 20, 9, 9, 5, 2, (1, 2)),
    "k = 7": ("fp32", 16, 9, 9, 7, 1, (3, 3)),
    "k = 1": ("bf16", 16, 9, 9, 1, 1, (0, 0)),
    "stride 3": ("fp32", 16, 9, 9, 3, 3, (0, 0)),
    "Ho < 1: 1 x 9 under the reference's stride-2 rule": ("fp32", 16, 1, 9, 3, 2, (0, 1)),
    "Ho < 1: two rows, no pad, 3 x 3 stride 2 (C's division truncates towards zero)": ("bf16", 16, 2, 9, 3, 2, (0, 0)),
    "Wo < 1: 5 x 5 on three unpadded columns": ("fp32", 16, 9, 3, 5, 1, (0, 0)),
}


def case(cid):
    return CASES[IDS.index(cid)]


def parse_instance(short):
    """'strip<3,1,16,32>' -> ('strip', 3, 1, 16, 32)."""
    name, args = short[:-1].split("<")
    return (name,) + tuple(int(a) for a in args.split(","))


def letter_of(short):
    return next(letter for letter, row in INSTANCES.items() if row[0] == short)


def full_tag(short, dtype, act, bias):
    """The symbol ``ops.last_kernel()`` reports for an instance (dw_lds_kernel carries act and bias as template arguments)."""
    name, k, s, th, tw = parse_instance(short)
    if name == "strip":
        return "void cf::dw_strip_kernel<%s, %d, %d, %d, %d>(cf::DwParams, cf::DwLdsGeom, int, int, int)" % (_T[dtype], k, s, th, tw)
    return "void cf::dw_lds_kernel<%s, %d, %d, %d, %d, %d, %s>(cf::DwParams, cf::DwLdsGeom)" % (
        _T[dtype], k, s, th, tw, {"none": 0, "swish": 1}[act], "true" if bias else "false")


def pads(k, s, pad):
    """(pad_lo, pad_hi) of a pad name, applied to both axes."""
    if pad == "same":
        p = max(k - s, 0)
        return (p // 2, p - p // 2)
    return (k // 2, k // 2)


def out_size(n, k, s, pad):
    return (n + pad[0] + pad[1] - k) // s + 1


def inputs(cid):
    """(x [B, C, H, W], w [C, 1, k, k], bias [C] or None) of a case, seeded from its id: standard-normal x, taps scaled by 0.3 (as the
    depthwise tests of tests/test_gpu_parity.py), standard-normal bias."""
    _, dtype, C, H, W, k, s, pad, act, bias, B = case(cid)[:11]
    rng = np.random.default_rng(int.from_bytes(cid.encode(), "little") % (1 << 63))
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((C, 1, k, k)) * 0.3).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32) if bias else None
    return x, w, b


def ref64(x, w, k, s, pad, act="swish", bias=None):
    """ZeroPad2d(pad) -> depthwise k x k, stride s -> + bias -> Swish, in float64 on the float32 inputs."""
    x64 = np.asarray(x, np.float64)
    B, C, H, W = x64.shape
    xp = np.zeros((B, C, H + pad[0] + pad[1], W + pad[0] + pad[1]))
    xp[:, :, pad[0]:pad[0] + H, pad[0]:pad[0] + W] = x64
    Ho, Wo = out_size(H, k, s, pad), out_size(W, k, s, pad)
    w64 = np.asarray(w, np.float64).reshape(C, k, k)
    y = np.zeros((B, C, Ho, Wo))
    for ky in range(k):
        for kx in range(k):
            y += xp[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] * w64[:, ky, kx].reshape(1, C, 1, 1)
    if bias is not None:
        y += np.asarray(bias, np.float64).reshape(1, C, 1, 1)
    return y / (1.0 + np.exp(-y)) if act == "swish" else y


def edges(a, Cc):
    """The slices of an [B, C, Ho, Wo] array on which the sweep asserts parity one by one, so that a failure names the edge."""
    return (("whole tensor", a), ("first output row", a[:, :, :1]), ("last output row", a[:, :, -1:]),
            ("first output column", a[:, :, :, :1]), ("last output column", a[:, :, :, -1:]), ("channels of the last chunk", a[:, -Cc:]))

"""The case table of tests/test_mbconv_sweep.py, as plain data, and the float64 restatement of an MBConv block it is checked against.

Importable without a GPU: tests/test_abi.py uses the table for the completeness check (every group of block shapes the geometry
functions accept has a case; every case lands in the group its row claims) and ties ``ref64`` to the oracle.

A case = (id, dtype, Cin, hid, Cout, k, stride, H, W, tag, tag under the dtype's product switch).  Cout = 0: the expand+depthwise
op (``ops.expand_dw``), else the fused block (``ops.mbconv``).  ``tag`` is the instance ``ops.last_kernel()`` must report, without
the "void cf::" / "(cf::MbParams)" frame and with T for the storage type.  The last column is what the same case must reach under
``CF_DW_MATRIX=0`` (bf16 cases: the v_dot2c family) or ``CF_F4_VARIANT=1`` (fp32 / fp32_split cases: mbconv_f32_kernel): None = the
same instance, "REFUSED" = no family serves the shape then (CenterFaceValueError, no launch).  Rows b2t / b3t / b4t / b4u are
"REFUSED" without a switch too: bf16 shapes whose hid only cf_mbconv.hip's own bf16 instances (HC = 32 / 48) divide.  They ran
there until this sweep found those instances 1.1 - 4.7 bounds off the emulation (other rounding points) and NaN at Cin = 24 / 56 /
88; ``mb_geometry`` now refuses them, and the cases stay to say so.

Ids: <row><map>.  Rows: f / s / b + the backbone block whose table row serves the shape (10 = layer1.0 ... 41 = layer4.1) in fp32 /
fp32_split / bf16; a third letter t / u / p / s = the row of a family the shape FALLS BACK to (MB_TILE where HC = 32 / 48 divides
hid and the first family's HC does not; MB_PX where the matrix-core kernel has no row; MB_SP at both widths); x / y = expand+dw in
fp32_split / bf16 (40 ... 60 = layer4.0 ... 6.0).  Maps (output size, T = the instance's tile): a = 1x1, b = (T_h + 3) x 1,
c = T - 1, d = T + 1 (four tiles, three of them edge tiles), e / f = further widths near the tile for rows with more hidden sizes
to visit.  Stride-2 rows alternate even and odd input sizes.  Over a row's cases: both Cin of its JX class, Cout at the top of its
n-block count and at the smallest partial block, hid = HC (where hid != Cin allows) and an odd multiple, hid = 16 / 48 for the rows
with a 16-channel tail round, chunks-per-workgroup + 1 hidden chunks for expdw_f32_kernel.
"""
import numpy as np

CASES = (
    ("f10a", "fp32", 16, 32, 32, 3, 2, 2, 3, "mbconv_kernel<T,3,2,1,false,4,2,32,4,16,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,false>"),
    ("f10b", "fp32", 16, 96, 32, 3, 2, 15, 2, "mbconv_kernel<T,3,2,1,false,4,2,32,4,16,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,false>"),
    ("f10c", "fp32", 16, 96, 8, 3, 2, 6, 30, "mbconv_kernel<T,3,2,1,false,4,2,32,4,16,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,false>"),
    ("f10d", "fp32", 16, 32, 8, 3, 2, 11, 35, "mbconv_kernel<T,3,2,1,false,4,2,32,4,16,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,false>"),
    ("f11a", "fp32", 24, 48, 24, 3, 1, 1, 1, "mbconv_kernel<T,3,1,1,true,8,3,48,8,16,true>", "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,false>"),
    ("f11b", "fp32", 24, 144, 24, 3, 1, 11, 1, "mbconv_kernel<T,3,1,1,true,8,3,48,8,16,true>", "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,false>"),
    ("f11c", "fp32", 24, 96, 24, 3, 1, 7, 15, "mbconv_kernel<T,3,1,1,true,8,3,48,8,16,true>", "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,false>"),
    ("f11d", "fp32", 24, 48, 24, 3, 1, 9, 17, "mbconv_kernel<T,3,1,1,true,8,3,48,8,16,true>", "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,false>"),
    ("f20a", "fp32", 24, 16, 32, 5, 2, 2, 3, "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>", None),
    ("f20b", "fp32", 24, 48, 32, 5, 2, 23, 2, "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>", "mbconv_f32_kernel<5,2,1,false,4,3,48,8,16,false,false>"),
    ("f20c", "fp32", 24, 48, 8, 5, 2, 14, 30, "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>", "mbconv_f32_kernel<5,2,1,false,4,3,48,8,16,false,false>"),
    ("f20d", "fp32", 24, 16, 8, 5, 2, 19, 35, "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>", None),
    ("f20e", "fp32", 24, 96, 32, 5, 2, 14, 37, "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>", "mbconv_f32_kernel<5,2,1,false,4,3,48,8,16,false,false>"),
    ("f21a", "fp32", 32, 64, 32, 5, 1, 1, 1, "mbconv_f32_kernel<5,1,1,true,4,4,32,8,16,false,false>", None),
    ("f21b", "fp32", 32, 96, 32, 5, 1, 11, 1, "mbconv_f32_kernel<5,1,1,true,4,4,32,8,16,false,false>", None),
    ("f21c", "fp32", 32, 96, 32, 5, 1, 7, 15, "mbconv_f32_kernel<5,1,1,true,4,4,32,8,16,false,false>", None),
    ("f21d", "fp32", 32, 64, 32, 5, 1, 9, 17, "mbconv_f32_kernel<5,1,1,true,4,4,32,8,16,false,false>", None),
    ("f2ta", "fp32", 32, 48, 32, 5, 1, 1, 1, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("f2tb", "fp32", 32, 144, 32, 5, 1, 11, 1, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("f2tc", "fp32", 32, 144, 32, 5, 1, 7, 15, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("f2td", "fp32", 32, 48, 32, 5, 1, 9, 17, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("f30a", "fp32", 32, 64, 64, 3, 2, 2, 3, "mbconv_kernel<T,3,2,2,false,8,4,32,8,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,false>"),
    ("f30b", "fp32", 32, 96, 64, 3, 2, 23, 2, "mbconv_kernel<T,3,2,2,false,8,4,32,8,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,false>"),
    ("f30c", "fp32", 32, 96, 40, 3, 2, 14, 30, "mbconv_kernel<T,3,2,2,false,8,4,32,8,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,false>"),
    ("f30d", "fp32", 32, 64, 40, 3, 2, 19, 35, "mbconv_kernel<T,3,2,2,false,8,4,32,8,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,false>"),
    ("f31a", "fp32", 64, 32, 64, 3, 1, 1, 1, "mbconv_kernel<T,3,1,2,true,4,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,false>"),
    ("f31b", "fp32", 64, 96, 64, 3, 1, 11, 1, "mbconv_kernel<T,3,1,2,true,4,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,false>"),
    ("f31c", "fp32", 64, 96, 64, 3, 1, 7, 15, "mbconv_kernel<T,3,1,2,true,4,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,false>"),
    ("f31d", "fp32", 64, 32, 64, 3, 1, 9, 17, "mbconv_kernel<T,3,1,2,true,4,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,false>"),
    ("f40a", "fp32", 64, 32, 96, 5, 1, 1, 1, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,false>"),
    ("f40b", "fp32", 64, 96, 96, 5, 1, 11, 1, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,false>"),
    ("f40c", "fp32", 64, 96, 72, 5, 1, 7, 15, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,false>"),
    ("f40d", "fp32", 64, 32, 72, 5, 1, 9, 17, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,false>"),
    ("f41a", "fp32", 96, 32, 96, 5, 1, 1, 1, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,false>"),
    ("f41b", "fp32", 96, 160, 96, 5, 1, 11, 1, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,false>"),
    ("f41c", "fp32", 96, 160, 96, 5, 1, 7, 15, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,false>"),
    ("f41d", "fp32", 96, 32, 96, 5, 1, 9, 17, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,false>"),
    ("s10a", "fp32_split", 16, 32, 32, 3, 2, 2, 3, "mbconv_f32_kernel<3,2,1,false,4,2,32,4,16,false,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,true>"),
    ("s10b", "fp32_split", 16, 96, 32, 3, 2, 15, 2, "mbconv_f32_kernel<3,2,1,false,4,2,32,4,16,false,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,true>"),
    ("s10c", "fp32_split", 16, 96, 8, 3, 2, 6, 30, "mbconv_f32_kernel<3,2,1,false,4,2,32,4,16,false,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,true>"),
    ("s10d", "fp32_split", 16, 32, 8, 3, 2, 11, 35, "mbconv_f32_kernel<3,2,1,false,4,2,32,4,16,false,true>", "mbconv_f32_kernel<3,2,1,false,4,2,32,8,16,false,true>"),
    ("s11a", "fp32_split", 24, 48, 24, 3, 1, 1, 1, "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,true>", None),
    ("s11b", "fp32_split", 24, 144, 24, 3, 1, 11, 1, "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,true>", None),
    ("s11c", "fp32_split", 24, 96, 24, 3, 1, 7, 15, "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,true>", None),
    ("s11d", "fp32_split", 24, 48, 24, 3, 1, 9, 17, "mbconv_f32_kernel<3,1,1,true,4,3,48,8,16,false,true>", None),
    ("s20a", "fp32_split", 24, 16, 32, 5, 2, 2, 3, "mbconv_f32_kernel<5,2,1,false,4,3,16,8,16,false,true>", "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>"),
    ("s20b", "fp32_split", 24, 48, 32, 5, 2, 23, 2, "mbconv_f32_kernel<5,2,1,false,4,3,16,8,16,false,true>", "mbconv_f32_kernel<5,2,1,false,4,3,48,8,16,false,true>"),
    ("s20c", "fp32_split", 24, 48, 8, 5, 2, 14, 30, "mbconv_f32_kernel<5,2,1,false,4,3,16,8,16,false,true>", "mbconv_f32_kernel<5,2,1,false,4,3,48,8,16,false,true>"),
    ("s20d", "fp32_split", 24, 16, 8, 5, 2, 19, 35, "mbconv_f32_kernel<5,2,1,false,4,3,16,8,16,false,true>", "mbconv_kernel<T,5,2,1,false,8,3,16,8,16,true>"),
    ("s20e", "fp32_split", 24, 96, 32, 5, 2, 14, 37, "mbconv_f32_kernel<5,2,1,false,4,3,16,8,16,false,true>", "mbconv_f32_kernel<5,2,1,false,4,3,48,8,16,false,true>"),
    ("s21a", "fp32_split", 32, 64, 32, 5, 1, 1, 1, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s21b", "fp32_split", 32, 96, 32, 5, 1, 11, 1, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s21c", "fp32_split", 32, 96, 32, 5, 1, 7, 15, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s21d", "fp32_split", 32, 64, 32, 5, 1, 9, 17, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s2ta", "fp32_split", 32, 48, 32, 5, 1, 1, 1, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("s2tb", "fp32_split", 32, 144, 32, 5, 1, 11, 1, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("s2tc", "fp32_split", 32, 144, 32, 5, 1, 7, 15, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("s2td", "fp32_split", 32, 48, 32, 5, 1, 9, 17, "mbconv_kernel<T,5,1,1,true,8,4,48,8,16,true>", None),
    ("s30a", "fp32_split", 32, 64, 64, 3, 2, 2, 3, "mbconv_kernel<T,3,2,2,false,4,4,32,4,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,true>"),
    ("s30b", "fp32_split", 32, 96, 64, 3, 2, 15, 2, "mbconv_kernel<T,3,2,2,false,4,4,32,4,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,true>"),
    ("s30c", "fp32_split", 32, 96, 40, 3, 2, 6, 30, "mbconv_kernel<T,3,2,2,false,4,4,32,4,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,true>"),
    ("s30d", "fp32_split", 32, 64, 40, 3, 2, 11, 35, "mbconv_kernel<T,3,2,2,false,4,4,32,4,16,true>", "mbconv_f32_kernel<3,2,2,false,4,4,32,8,16,false,true>"),
    ("s31a", "fp32_split", 64, 32, 64, 3, 1, 1, 1, "mbconv_kernel<T,3,1,2,true,8,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,true>"),
    ("s31b", "fp32_split", 64, 96, 64, 3, 1, 11, 1, "mbconv_kernel<T,3,1,2,true,8,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,true>"),
    ("s31c", "fp32_split", 64, 96, 64, 3, 1, 7, 15, "mbconv_kernel<T,3,1,2,true,8,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,true>"),
    ("s31d", "fp32_split", 64, 32, 64, 3, 1, 9, 17, "mbconv_kernel<T,3,1,2,true,8,8,32,8,16,true>", "mbconv_f32_kernel<3,1,2,true,4,8,32,8,16,true,true>"),
    ("s40a", "fp32_split", 64, 32, 96, 5, 1, 1, 1, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,true>"),
    ("s40b", "fp32_split", 64, 96, 96, 5, 1, 11, 1, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,true>"),
    ("s40c", "fp32_split", 64, 96, 72, 5, 1, 7, 15, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,true>"),
    ("s40d", "fp32_split", 64, 32, 72, 5, 1, 9, 17, "mbconv_kernel<T,5,1,3,false,8,8,32,8,16,true>", "mbconv_f32_kernel<5,1,3,false,4,8,32,8,16,true,true>"),
    ("s41a", "fp32_split", 96, 32, 96, 5, 1, 1, 1, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,true>"),
    ("s41b", "fp32_split", 96, 160, 96, 5, 1, 11, 1, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,true>"),
    ("s41c", "fp32_split", 96, 160, 96, 5, 1, 7, 15, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,true>"),
    ("s41d", "fp32_split", 96, 32, 96, 5, 1, 9, 17, "mbconv_kernel<T,5,1,3,true,4,12,32,8,16,true>", "mbconv_f32_kernel<5,1,3,true,4,12,32,8,16,true,true>"),
    ("s2sa", "fp32_split", 24, 32, 24, 5, 1, 1, 1, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s2sb", "fp32_split", 32, 96, 32, 5, 1, 11, 1, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s2sc", "fp32_split", 24, 96, 24, 5, 1, 7, 15, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("s2sd", "fp32_split", 32, 160, 32, 5, 1, 9, 17, "mbconv6_kernel<5,1,32,8,16,4,8,true,4>", None),
    ("x40a", "fp32_split", 64, 32, 0, 5, 1, 1, 1, "expdw_f32_kernel<5,1,32,10,40,8,8,true,true,true,2>", None),
    ("x40b", "fp32_split", 64, 416, 0, 5, 1, 13, 1, "expdw_f32_kernel<5,1,32,10,40,8,8,true,true,true,2>", None),
    ("x40c", "fp32_split", 64, 416, 0, 5, 1, 9, 39, "expdw_f32_kernel<5,1,32,10,40,8,8,true,true,true,2>", None),
    ("x40d", "fp32_split", 64, 32, 0, 5, 1, 11, 41, "expdw_f32_kernel<5,1,32,10,40,8,8,true,true,true,2>", None),
    ("x41a", "fp32_split", 96, 32, 0, 5, 1, 1, 1, "expdw_f32_kernel<5,1,32,10,40,12,8,false,true,true,2>", None),
    ("x41b", "fp32_split", 96, 608, 0, 5, 1, 13, 1, "expdw_f32_kernel<5,1,32,10,40,12,8,false,true,true,2>", None),
    ("x41c", "fp32_split", 96, 608, 0, 5, 1, 9, 39, "expdw_f32_kernel<5,1,32,10,40,12,8,false,true,true,2>", None),
    ("x41d", "fp32_split", 96, 32, 0, 5, 1, 11, 41, "expdw_f32_kernel<5,1,32,10,40,12,8,false,true,true,2>", None),
    ("x50a", "fp32_split", 96, 32, 0, 5, 2, 2, 3, "expdw_f32_kernel<5,2,32,5,20,12,8,false,true,true,2>", None),
    ("x50b", "fp32_split", 96, 608, 0, 5, 2, 17, 2, "expdw_f32_kernel<5,2,32,5,20,12,8,false,true,true,2>", None),
    ("x50c", "fp32_split", 96, 608, 0, 5, 2, 8, 38, "expdw_f32_kernel<5,2,32,5,20,12,8,false,true,true,2>", None),
    ("x50d", "fp32_split", 96, 32, 0, 5, 2, 13, 43, "expdw_f32_kernel<5,2,32,5,20,12,8,false,true,true,2>", None),
    ("x51a", "fp32_split", 160, 32, 0, 5, 1, 1, 1, "expdw_f32_kernel<5,1,32,10,20,20,12,false,true,true,3>", None),
    ("x51b", "fp32_split", 160, 352, 0, 5, 1, 13, 1, "expdw_f32_kernel<5,1,32,10,20,20,12,false,true,true,3>", None),
    ("x51c", "fp32_split", 160, 352, 0, 5, 1, 9, 19, "expdw_f32_kernel<5,1,32,10,20,20,12,false,true,true,3>", None),
    ("x51d", "fp32_split", 160, 32, 0, 5, 1, 11, 21, "expdw_f32_kernel<5,1,32,10,20,20,12,false,true,true,3>", None),
    ("x60a", "fp32_split", 160, 32, 0, 3, 1, 1, 1, "expdw_f32_kernel<3,1,32,10,20,20,8,true,true,true,2>", None),
    ("x60b", "fp32_split", 160, 352, 0, 3, 1, 13, 1, "expdw_f32_kernel<3,1,32,10,20,20,8,true,true,true,2>", None),
    ("x60c", "fp32_split", 160, 352, 0, 3, 1, 9, 19, "expdw_f32_kernel<3,1,32,10,20,20,8,true,true,true,2>", None),
    ("x60d", "fp32_split", 160, 32, 0, 3, 1, 11, 21, "expdw_f32_kernel<3,1,32,10,20,20,8,true,true,true,2>", None),
    ("b10a", "bf16", 8, 32, 32, 3, 2, 2, 3, "mbconv_px_kernel<3,2,1,false,4,1,32,8,16>", None),
    ("b10b", "bf16", 16, 96, 32, 3, 2, 23, 2, "mbconv_px_kernel<3,2,1,false,4,1,32,8,16>", None),
    ("b10c", "bf16", 8, 96, 8, 3, 2, 14, 30, "mbconv_px_kernel<3,2,1,false,4,1,32,8,16>", None),
    ("b10d", "bf16", 16, 32, 8, 3, 2, 19, 35, "mbconv_px_kernel<3,2,1,false,4,1,32,8,16>", None),
    ("b11a", "bf16", 24, 16, 24, 3, 1, 1, 1, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>", "REFUSED"),
    ("b11b", "bf16", 32, 48, 32, 3, 1, 19, 1, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>", "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>"),
    ("b11c", "bf16", 24, 144, 24, 3, 1, 15, 15, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>", "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>"),
    ("b11d", "bf16", 32, 48, 32, 3, 1, 17, 17, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>", "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>"),
    ("b11e", "bf16", 24, 16, 24, 3, 1, 15, 18, "mbconv_mx_kernel<3,2,2,true,16,16,4,true,false,true,false>", "REFUSED"),
    ("b1pa", "bf16", 24, 96, 24, 3, 1, 1, 1, "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>", None),
    ("b1pb", "bf16", 32, 288, 32, 3, 1, 19, 1, "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>", None),
    ("b1pc", "bf16", 24, 288, 24, 3, 1, 15, 15, "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>", None),
    ("b1pd", "bf16", 32, 96, 32, 3, 1, 17, 17, "mbconv_px_kernel<3,1,1,true,4,2,48,16,16>", None),
    ("b20a", "bf16", 24, 16, 32, 5, 2, 2, 3, "mbconv_mx2_kernel<5,2,2,8,16,true,false,false>", "REFUSED"),
    ("b20b", "bf16", 32, 48, 32, 5, 2, 23, 2, "mbconv_mx2_kernel<5,2,2,8,16,true,false,false>", "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>"),
    ("b20c", "bf16", 24, 144, 8, 5, 2, 14, 30, "mbconv_mx2_kernel<5,2,2,8,16,true,false,false>", "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>"),
    ("b20d", "bf16", 32, 48, 8, 5, 2, 19, 35, "mbconv_mx2_kernel<5,2,2,8,16,true,false,false>", "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>"),
    ("b20e", "bf16", 24, 16, 32, 5, 2, 14, 37, "mbconv_mx2_kernel<5,2,2,8,16,true,false,false>", "REFUSED"),
    ("b2pa", "bf16", 24, 96, 32, 5, 2, 2, 3, "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>", None),
    ("b2pb", "bf16", 32, 288, 32, 5, 2, 23, 2, "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>", None),
    ("b2pc", "bf16", 24, 288, 8, 5, 2, 14, 14, "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>", None),
    ("b2pd", "bf16", 32, 96, 8, 5, 2, 19, 19, "mbconv_px_kernel<5,2,1,false,3,2,48,8,8>", None),
    ("b21a", "bf16", 24, 32, 24, 5, 1, 1, 1, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>", "REFUSED"),
    ("b21b", "bf16", 32, 96, 32, 5, 1, 19, 1, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>", "REFUSED"),
    ("b21c", "bf16", 24, 64, 24, 5, 1, 15, 15, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>", "mbconv_px_kernel<5,1,1,true,4,2,64,8,16>"),
    ("b21d", "bf16", 32, 192, 32, 5, 1, 17, 17, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>", "mbconv_px_kernel<5,1,1,true,4,2,64,8,16>"),
    ("b21e", "bf16", 24, 32, 24, 5, 1, 15, 18, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>", "REFUSED"),
    ("b21f", "bf16", 32, 96, 32, 5, 1, 18, 15, "mbconv_mx_kernel<5,2,2,true,16,16,4,false,false,true,false>", "REFUSED"),
    ("b2ta", "bf16", 24, 48, 24, 5, 1, 1, 1, "REFUSED", None),
    ("b2tb", "bf16", 32, 144, 32, 5, 1, 11, 1, "REFUSED", None),
    ("b2tc", "bf16", 24, 144, 24, 5, 1, 7, 15, "REFUSED", None),
    ("b2td", "bf16", 32, 48, 32, 5, 1, 9, 17, "REFUSED", None),
    ("b30a", "bf16", 24, 32, 64, 3, 2, 2, 3, "mbconv_px_kernel<3,2,2,false,4,2,32,8,16>", None),
    ("b30b", "bf16", 32, 96, 64, 3, 2, 23, 2, "mbconv_px_kernel<3,2,2,false,4,2,32,8,16>", None),
    ("b30c", "bf16", 24, 96, 40, 3, 2, 14, 30, "mbconv_px_kernel<3,2,2,false,4,2,32,8,16>", None),
    ("b30d", "bf16", 32, 160, 40, 3, 2, 19, 35, "mbconv_px_kernel<3,2,2,false,4,2,32,8,16>", None),
    ("b31a", "bf16", 56, 64, 56, 3, 1, 1, 1, "mbconv_px_kernel<3,1,2,true,4,4,64,8,16>", None),
    ("b31b", "bf16", 64, 192, 64, 3, 1, 11, 1, "mbconv_px_kernel<3,1,2,true,4,4,64,8,16>", None),
    ("b31c", "bf16", 56, 192, 56, 3, 1, 7, 15, "mbconv_px_kernel<3,1,2,true,4,4,64,8,16>", None),
    ("b31d", "bf16", 64, 128, 64, 3, 1, 9, 17, "mbconv_px_kernel<3,1,2,true,4,4,64,8,16>", None),
    ("b3ta", "bf16", 56, 32, 56, 3, 1, 1, 1, "REFUSED", None),
    ("b3tb", "bf16", 64, 96, 64, 3, 1, 11, 1, "REFUSED", None),
    ("b3tc", "bf16", 56, 96, 56, 3, 1, 7, 15, "REFUSED", None),
    ("b3td", "bf16", 64, 32, 64, 3, 1, 9, 17, "REFUSED", None),
    ("b40a", "bf16", 56, 64, 96, 5, 1, 1, 1, "mbconv_px_kernel<5,1,3,false,4,4,64,8,16>", None),
    ("b40b", "bf16", 64, 192, 96, 5, 1, 11, 1, "mbconv_px_kernel<5,1,3,false,4,4,64,8,16>", None),
    ("b40c", "bf16", 56, 192, 72, 5, 1, 7, 15, "mbconv_px_kernel<5,1,3,false,4,4,64,8,16>", None),
    ("b40d", "bf16", 64, 128, 72, 5, 1, 9, 17, "mbconv_px_kernel<5,1,3,false,4,4,64,8,16>", None),
    ("b4ta", "bf16", 56, 32, 96, 5, 1, 1, 1, "REFUSED", None),
    ("b4tb", "bf16", 64, 96, 96, 5, 1, 11, 1, "REFUSED", None),
    ("b4tc", "bf16", 56, 96, 72, 5, 1, 7, 19, "REFUSED", None),
    ("b4td", "bf16", 64, 32, 72, 5, 1, 9, 21, "REFUSED", None),
    ("b41a", "bf16", 88, 64, 88, 5, 1, 1, 1, "mbconv_px_kernel<5,1,3,true,4,6,64,8,16>", None),
    ("b41b", "bf16", 96, 192, 96, 5, 1, 11, 1, "mbconv_px_kernel<5,1,3,true,4,6,64,8,16>", None),
    ("b41c", "bf16", 88, 192, 88, 5, 1, 7, 15, "mbconv_px_kernel<5,1,3,true,4,6,64,8,16>", None),
    ("b41d", "bf16", 96, 64, 96, 5, 1, 9, 17, "mbconv_px_kernel<5,1,3,true,4,6,64,8,16>", None),
    ("b4ua", "bf16", 88, 32, 88, 5, 1, 1, 1, "REFUSED", None),
    ("b4ub", "bf16", 96, 160, 96, 5, 1, 11, 1, "REFUSED", None),
    ("b4uc", "bf16", 88, 160, 88, 5, 1, 7, 19, "REFUSED", None),
    ("b4ud", "bf16", 96, 32, 96, 5, 1, 9, 21, "REFUSED", None),
    ("y40a", "bf16", 56, 32, 0, 5, 1, 1, 1, "expdw_mx_kernel<5,4,10,40,8,true>", "expdw_px_kernel<5,1,4,32,10,40>"),
    ("y40b", "bf16", 64, 96, 0, 5, 1, 13, 1, "expdw_mx_kernel<5,4,10,40,8,true>", "expdw_px_kernel<5,1,4,32,10,40>"),
    ("y40c", "bf16", 56, 96, 0, 5, 1, 9, 39, "expdw_mx_kernel<5,4,10,40,8,true>", "expdw_px_kernel<5,1,4,32,10,40>"),
    ("y40d", "bf16", 64, 32, 0, 5, 1, 11, 41, "expdw_mx_kernel<5,4,10,40,8,true>", "expdw_px_kernel<5,1,4,32,10,40>"),
    ("y41a", "bf16", 88, 32, 0, 5, 1, 1, 1, "expdw_mx_kernel<5,6,10,40,8,true>", "expdw_px_kernel<5,1,6,32,10,40>"),
    ("y41b", "bf16", 96, 160, 0, 5, 1, 13, 1, "expdw_mx_kernel<5,6,10,40,8,true>", "expdw_px_kernel<5,1,6,32,10,40>"),
    ("y41c", "bf16", 88, 160, 0, 5, 1, 9, 39, "expdw_mx_kernel<5,6,10,40,8,true>", "expdw_px_kernel<5,1,6,32,10,40>"),
    ("y41d", "bf16", 96, 32, 0, 5, 1, 11, 41, "expdw_mx_kernel<5,6,10,40,8,true>", "expdw_px_kernel<5,1,6,32,10,40>"),
    ("y50a", "bf16", 88, 32, 0, 5, 2, 2, 3, "expdw_px_kernel<5,2,6,32,10,20>", None),
    ("y50b", "bf16", 96, 160, 0, 5, 2, 27, 2, "expdw_px_kernel<5,2,6,32,10,20>", None),
    ("y50c", "bf16", 88, 160, 0, 5, 2, 18, 38, "expdw_px_kernel<5,2,6,32,10,20>", None),
    ("y50d", "bf16", 96, 32, 0, 5, 2, 23, 43, "expdw_px_kernel<5,2,6,32,10,20>", None),
    ("y51a", "bf16", 152, 32, 0, 5, 1, 1, 1, "expdw_mx_kernel<5,10,20,20,4,false>", "expdw_px_kernel<5,1,10,32,10,20>"),
    ("y51b", "bf16", 160, 96, 0, 5, 1, 23, 1, "expdw_mx_kernel<5,10,20,20,4,false>", "expdw_px_kernel<5,1,10,32,10,20>"),
    ("y51c", "bf16", 152, 96, 0, 5, 1, 19, 19, "expdw_mx_kernel<5,10,20,20,4,false>", "expdw_px_kernel<5,1,10,32,10,20>"),
    ("y51d", "bf16", 160, 32, 0, 5, 1, 21, 21, "expdw_mx_kernel<5,10,20,20,4,false>", "expdw_px_kernel<5,1,10,32,10,20>"),
    ("y60a", "bf16", 152, 32, 0, 3, 1, 1, 1, "expdw_mx_kernel<3,10,10,20,4,true>", "expdw_px_kernel<3,1,10,32,10,20>"),
    ("y60b", "bf16", 160, 96, 0, 3, 1, 13, 1, "expdw_mx_kernel<3,10,10,20,4,true>", "expdw_px_kernel<3,1,10,32,10,20>"),
    ("y60c", "bf16", 152, 96, 0, 3, 1, 9, 19, "expdw_mx_kernel<3,10,10,20,4,true>", "expdw_px_kernel<3,1,10,32,10,20>"),
    ("y60d", "bf16", 160, 32, 0, 3, 1, 11, 21, "expdw_mx_kernel<3,10,10,20,4,true>", "expdw_px_kernel<3,1,10,32,10,20>"),
)

IDS = tuple(c[0] for c in CASES)
SWITCH = {"bf16": ("CF_DW_MATRIX", "0"), "fp32": ("CF_F4_VARIANT", "1"), "fp32_split": ("CF_F4_VARIANT", "1")}      # dtype -> its product switch
_T = {"bf16": "unsigned short", "fp32": "float", "fp32_split": "sp32_t"}
# tag prefix -> family (ops.MB_KINDS names), for the completeness check
FAMILY = {"mbconv_kernel": "MB_TILE", "mbconv_px_kernel": "MB_PX", "expdw_px_kernel": "XD_PX", "expdw_mx_kernel": "XD_MX", "mbconv_mx_kernel": "MB_MX",
          "mbconv_mx2_kernel": "MB_MX2", "mbconv_f32_kernel": "MB_F32", "expdw_f32_kernel": "XD_F32", "mbconv6_kernel": "MB_SP"}


def case(cid):
    return CASES[IDS.index(cid)]


def short_tag(c, env):
    """The tag column that applies under the environment ``env`` (a mapping): the switch column when the dtype's switch is set."""
    name, value = SWITCH[c[1]]
    return c[10] if (c[10] is not None and env.get(name) == value) else c[9]


def full_tag(short, dtype):
    """'mbconv_kernel<T,3,2,1,false,4,2,32,4,16,true>' -> the symbol ``ops.last_kernel()`` reports."""
    name, args = short[:-1].split("<")
    return "void cf::%s<%s>(cf::MbParams)" % (name, ", ".join(_T[dtype] if a == "T" else a for a in args.split(",")))


def family(short):
    return None if short == "REFUSED" else FAMILY[short.split("<")[0]]


# where a family's tag carries (k, stride, JX, HC, n-blocks or 2 n-blocks, residual, tail): template argument positions, or a constant
_ARGS = {"MB_TILE": dict(k=1, s=2, nbo=3, res=4, JX=6, HC=7), "MB_PX": dict(k=0, s=1, nbo=2, res=3, JX=5, HC=6), "XD_PX": dict(k=0, s=1, JX=2, HC=3),
         "XD_MX": dict(k=0, JX=1), "MB_MX": dict(k=0, JX=1, nmb=2, res=3, tail=7), "MB_MX2": dict(k=0, JX=1, nmb=2, tail=5),
         "MB_F32": dict(k=0, s=1, nbo=2, res=3, JX=5, HC=6), "XD_F32": dict(k=0, s=1, HC=2, JX=5), "MB_SP": dict(k=0, s=1, HC=2, JX=5, res=7)}
_FIXED = {"XD_MX": dict(s=1, HC=32), "MB_MX": dict(s=1, HC=32), "MB_MX2": dict(s=2, HC=32, res=0), "MB_SP": dict(nbo=1)}


def claimed(short):
    """What a tag says about the table row it names: family, k, s, JX, HC and -- where the family's template carries them --
    n-blocks, residual, tail."""
    fam = family(short)
    args = short[:-1].split("<")[1].split(",")
    out = dict(kind=fam, **_FIXED.get(fam, {}))
    for name, pos in _ARGS[fam].items():
        v = args[pos]
        out[name] = int(v == "true") if v in ("true", "false") else int(v)
    if "nmb" in out:
        out["nbo"] = out.pop("nmb") // 2
    return out


# shapes no family serves: (dtype, Cin, hid, Cout, k, stride); Cout = 0 = the expand+depthwise op
REFUSED = {
    "Cin % 8": ("fp32", 12, 72, 24, 3, 1),
    "Cout > 96": ("bf16", 64, 384, 104, 5, 1),
    "hid == Cin": ("fp32_split", 32, 32, 32, 5, 1),
    "hid no multiple of a serving HC (bf16)": ("bf16", 16, 40, 24, 3, 2),
    "hid no multiple of a serving HC (fp32)": ("fp32", 64, 80, 64, 3, 1),
    "k = 7": ("fp32", 16, 96, 24, 7, 2),
    "stride = 3": ("bf16", 16, 96, 24, 3, 3),
    "expand+dw in fp32": ("fp32", 96, 576, 0, 5, 2),
    "expand+dw, hid no multiple of HC": ("bf16", 96, 80, 0, 5, 2),
}


def group_key(dtype, pick, Cin, hid, Cout, k, s):
    """The class of block shapes one table row serves: (dtype, family, k, s, JX, n-blocks, residual, 16-channel tail, HC)."""
    return (dtype, pick["kind"], k, s, pick["JX"], (Cout + 31) // 32, int(Cin == Cout and s == 1), int(hid % 32 == 16), pick["HC"])


def out_size(n, k, s):
    return (n + max(k - s, 0) - k) // s + 1


def weights(rng, Cin, hid, Cout, k):
    """Seeded weights scaled so that every activation of the block stays O(1) (tests/test_gpu_parity.py's multi-tile test)."""
    we = (rng.standard_normal((hid, Cin)) * 1.5 / np.sqrt(Cin)).astype(np.float32)
    wd = (rng.standard_normal((hid, 1, k, k)) * 1.5 / k).astype(np.float32)
    wp = (rng.standard_normal((Cout, hid)) / np.sqrt(hid)).astype(np.float32) if Cout else None
    return we, wd, wp


def _swish64(v):
    return v / (1.0 + np.exp(-v))


def ref64(x, we, wd, wp, k, s):
    """MBConvBlock.forward (se off, no BN) restated in float64 on the float32 inputs: expand 1x1 -> swish -> depthwise k x k with
    the project's same-padding (k - s zeros in all, (k - s) // 2 of them in front) -> swish -> project 1x1 (+ x when Cin == Cout and
    s == 1).  ``wp`` None: stop after the second swish (the expand+depthwise op)."""
    x64 = x.astype(np.float64)
    B, Cin, H, W = x.shape
    hid = we.shape[0]
    e = _swish64(np.einsum("bchw,nc->bnhw", x64, we.reshape(hid, Cin).astype(np.float64), optimize=True))
    pad = max(k - s, 0)
    lo = pad // 2
    ep = np.zeros((B, hid, H + pad, W + pad))
    ep[:, :, lo:lo + H, lo:lo + W] = e
    Ho, Wo = out_size(H, k, s), out_size(W, k, s)
    w64 = wd.reshape(hid, k, k).astype(np.float64)
    d = np.zeros((B, hid, Ho, Wo))
    for ky in range(k):
        for kx in range(k):
            d += ep[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] * w64[:, ky, kx].reshape(1, hid, 1, 1)
    d = _swish64(d)
    if wp is None:
        return d
    Cout = wp.shape[0]
    y = np.einsum("bnhw,on->bohw", d, wp.reshape(Cout, hid).astype(np.float64), optimize=True)
    return y + x64 if (Cin == Cout and s == 1) else y

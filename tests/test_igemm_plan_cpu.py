"""The implicit-GEMM launch planner (``csrc/kernels/igemm_plan.h``) on the host: the
stand-alone ``csrc/kernels/igemm_plan_check.cpp`` is built with the host compiler, plain and
with AddressSanitizer + UndefinedBehaviorSanitizer, and

* its sweep (M x N x channels x taps x stride phases x operand width x B layout x split
  allowed x switches x every tile the tuner would accept) finds every plan inside the limits
  the kernels and the callers state: a tile of the family's table, grid and split cover,
  split partials inside the workspace the sizing functions give, statistics-slab rows inside
  the slab, the uniform-tap / padded-K / second-source / incremental conditions, one tuner key
  per shape;
* the dispatch it prints for the model zoo (the 26 launches of ``test_conv_args_cpu.py``, the
  linear heads, the stride-2 dgrads with and without their shortcut, the weight gradients) at
  batch 32 and 3 under engine 0, 1 and 2 is the table below - recorded from the launch code
  as it was before the planner existed (its host sections against stubbed launch entry points:
  kernel symbol, grid, block, the argument fields, the follow-up launch, the sizing
  functions and the tuner key of every launch), so a change of kernel, tile, split count or
  key for one of these layers shows here, on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "csrc", "kernels")

# shape engine : kernel<template arguments> grid, block, K tiles per split, tiles, K (padded)
# | the split-K finalize / split reduce launch | statistics-slab rows (where asked for) |
# workspace floats | tuner key (LDS-DMA launches).  igemm_rows_kernel<BM, BN, WM, WN, VW, BKC,
# SPLIT>, igemm_rows_dma(_uni)_kernel<BM, BN, WM, WN, BKC, SPLIT, PH>, igemm_wgrad_kernel<BM,
# BN, WM, WN, VWA, VWB>, igemm_wgrad_dma(_inc)_kernel<BM, BN, WM, WN>.  "halo": the 3x3 halo
# path takes the launch; "apart": no merged launch reads a second source
# there (the caller runs the two dgrads apart); a strided dgrad off the LDS-DMA engine is one
# launch per phase.
ZOO = """\
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 1568,1,1 block 256 kps 13 tiles_n 1 tiles_total 1568 Ktot 392 kpad 0 | none | slab_rows 1568 | ws 0 | -
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 1568,1,1 block 256 kps 13 tiles_n 1 tiles_total 1568 Ktot 392 kpad 0 | none | slab_rows 1568 | ws 0 | -
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 0: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 3136,1,1 block 256 kps 18 tiles_n 1 tiles_total 3136 Ktot 576 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 1: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 3136,1,1 block 256 kps 24 tiles_n 1 tiles_total 3136 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 2: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 3136,1,1 block 256 kps 24 tiles_n 1 tiles_total 3136 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 3: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 3136,1,1 block 256 kps 32 tiles_n 1 tiles_total 3136 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
wgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 4,1,128 block 256 kps 98 tiles_n 4 tiles_total 4 | wgrad_reduce_kernel grid 98 | ws 6422528 | -
fwd n32 56x56 c64 k64 3x3 s1,1 p1,1 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 392,1,1 block 256 kps 18 tiles_n 1 tiles_total 392 Ktot 576 kpad 0 | none | slab_rows 392 | ws 0 | -
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 392,1,1 block 256 kps 18 tiles_n 1 tiles_total 392 Ktot 576 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, false, false> grid 392,1,1 block 256 kps 18 tiles_n 1 tiles_total 392 Ktot 576 kpad 0 | none | slab_rows - | ws 0 | -
wgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 5,1,102 block 256 kps 31 tiles_n 5 tiles_total 5 | wgrad_reduce_kernel grid 144 | ws 6119424 | -
fwd n32 56x56 c64 k128 3x3 s2,2 p1,1 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 196,1,2 block 256 kps 9 tiles_n 1 tiles_total 196 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 6422528 | -
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 0: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 98,1,1 block 256 kps 4 tiles_n 1 tiles_total 98 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 1: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 98,1,1 block 256 kps 8 tiles_n 1 tiles_total 98 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 2: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 98,1,1 block 256 kps 8 tiles_n 1 tiles_total 98 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 3: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 98,1,1 block 256 kps 16 tiles_n 1 tiles_total 98 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
pair n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e0 : apart
fwd n32 56x56 c64 k128 1x1 s2,2 p0,0 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 196,1,1 block 256 kps 2 tiles_n 1 tiles_total 196 Ktot 64 kpad 0 | none | slab_rows 196 | ws 0 | -
dgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 wt1 e0 : phase 0: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 98,1,1 block 256 kps 4 tiles_n 1 tiles_total 98 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | -
fwd n32 17x17 c128 k128 1x7 s1,1 p0,3 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 73,1,3 block 256 kps 10 tiles_n 1 tiles_total 73 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 3551232 | -
dgrad n32 17x17 c128 k128 1x7 s1,1 p0,3 wt1 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 73,1,3 block 256 kps 10 tiles_n 1 tiles_total 73 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows - | ws 3551232 | -
fwd n32 17x17 c128 k192 7x1 s1,1 p3,0 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 111,1,3 block 256 kps 10 tiles_n 3 tiles_total 111 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 3,256 | slab_rows 256 | ws 5326848 | -
dgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 wt1 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 73,1,5 block 256 kps 9 tiles_n 1 tiles_total 73 Ktot 1344 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows - | ws 5918720 | -
fwd n32 35x35 c288 k384 3x3 s2,2 p0,0 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 219,1,3 block 256 kps 27 tiles_n 3 tiles_total 219 Ktot 2592 kpad 0 | splitk_finalize_kernel<64> grid 6,171 | slab_rows 171 | ws 10653696 | -
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 243,1,1 block 256 kps 48 tiles_n 3 tiles_total 243 Ktot 1536 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 231,1,1 block 256 kps 24 tiles_n 3 tiles_total 231 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 231,1,1 block 256 kps 24 tiles_n 3 tiles_total 231 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 219,1,1 block 256 kps 12 tiles_n 3 tiles_total 219 Ktot 384 kpad 0 | none | slab_rows - | ws 0 | -
fwd n32 35x35 c48 k64 5x5 s1,1 p2,2 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 154,1,4 block 256 kps 10 tiles_n 1 tiles_total 154 Ktot 1200 kpad 0 | splitk_finalize_kernel<64> grid 1,307 | slab_rows 307 | ws 10035200 | -
dgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 154,1,4 block 256 kps 13 tiles_n 1 tiles_total 154 Ktot 1600 kpad 0 | splitk_finalize_kernel<64> grid 1,307 | slab_rows - | ws 7526400 | -
fwd n32 56x56 c128 k128 1x1 s1,1 p0,0 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 784,1,1 block 256 kps 4 tiles_n 1 tiles_total 784 Ktot 128 kpad 0 | none | slab_rows 784 | ws 0 | -
pointwise n32 56x56 c128 k64 ldb128 tapmap1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 392,1,1 block 256 kps 4 tiles_n 1 tiles_total 392 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | -
pointwise n32 1x1 c512 k1000 ldb512 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 8,1,2 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 512 kpad 0 | splitk_finalize_kernel<64> grid 16,4 | slab_rows - | ws 64000 | -
pointwise n32 1x1 c1000 k512 ldb512 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, false, true> grid 4,1,4 block 256 kps 8 tiles_n 4 tiles_total 4 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 8,4 | slab_rows - | ws 65536 | -
wgrad n32 1x1 c512 k1000 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 32,1,1 block 256 kps 1 tiles_n 4 tiles_total 32 | none | ws 0 | -
pointwise n32 1x1 c2048 k1000 ldb2048 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 8,1,8 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 2048 kpad 0 | splitk_finalize_kernel<64> grid 16,4 | slab_rows - | ws 256000 | -
pointwise n32 1x1 c1000 k2048 ldb2048 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, false, true> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,4 | slab_rows - | ws 262144 | -
pointwise n32 1x1 c1000 k2048 ldb1000 tapmap1 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,4 | slab_rows - | ws 262144 | -
wgrad n32 1x1 c2048 k1000 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 128,1,1 block 256 kps 1 tiles_n 16 tiles_total 128 | none | ws 0 | -
pointwise n32 1x1 c512 k64500 ldb512 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 504,1,1 block 256 kps 16 tiles_n 504 tiles_total 504 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
pointwise n32 1x1 c64500 k512 ldb64500 tapmap1 e0 : igemm_rows_kernel<128, 128, 2, 2, 4, true, true> grid 4,1,63 block 256 kps 32 tiles_n 4 tiles_total 4 Ktot 64500 kpad 0 | splitk_finalize_kernel<64> grid 8,4 | slab_rows - | ws 1032192 | -
wgrad n32 1x1 c512 k64500 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 4, 8> grid 2016,1,1 block 256 kps 1 tiles_n 4 tiles_total 2016 | none | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 49,1,1 block 256 kps 8 tiles_n 1 tiles_total 49 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 49,1,1 block 256 kps 16 tiles_n 1 tiles_total 49 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 49,1,1 block 256 kps 16 tiles_n 1 tiles_total 49 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 49,1,1 block 256 kps 32 tiles_n 1 tiles_total 49 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
pair n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e0 : apart
dgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 26,1,1 block 256 kps 16 tiles_n 2 tiles_total 26 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 26,1,1 block 256 kps 32 tiles_n 2 tiles_total 26 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 26,1,1 block 256 kps 32 tiles_n 2 tiles_total 26 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 26,1,1 block 256 kps 64 tiles_n 2 tiles_total 26 Ktot 2048 kpad 0 | none | slab_rows - | ws 0 | -
pair n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e0 : apart
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 49,1,1 block 256 kps 8 tiles_n 1 tiles_total 49 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 49,1,1 block 256 kps 16 tiles_n 1 tiles_total 49 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 49,1,1 block 256 kps 16 tiles_n 1 tiles_total 49 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 49,1,1 block 256 kps 32 tiles_n 1 tiles_total 49 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
bnred n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : not available
bnred n32 56x56 c64 k64 1x1 s1,1 p0,0 wt1 e0 : not available
bnred n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e0 : not available
wgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 5,1,49 block 256 kps 16 tiles_n 5 tiles_total 5 | wgrad_reduce_kernel grid 288 | ws 3612672 | -
wgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 1,1,49 block 256 kps 16 tiles_n 1 tiles_total 1 | wgrad_reduce_kernel grid 32 | ws 401408 | -
wgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 72,1,3 block 256 kps 17 tiles_n 18 tiles_total 72 | wgrad_reduce_kernel grid 4608 | ws 3538944 | -
wgrad n32 14x14 c256 k512 1x1 s2,2 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 8,1,3 block 256 kps 17 tiles_n 2 tiles_total 8 | wgrad_reduce_kernel grid 512 | ws 393216 | -
wgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 14,1,17 block 256 kps 17 tiles_n 7 tiles_total 14 | wgrad_reduce_kernel grid 672 | ws 2924544 | -
wgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 10,1,52 block 256 kps 24 tiles_n 10 tiles_total 10 | wgrad_reduce_kernel grid 300 | ws 5606400 | -
wgrad n32 56x56 c256 k64 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 2,1,196 block 256 kps 16 tiles_n 2 tiles_total 2 | wgrad_reduce_kernel grid 64 | ws 3211264 | -
fwd n3 224x224 c8 k64 7x7 s2,2 p3,3 stap1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 147,1,1 block 256 kps 13 tiles_n 1 tiles_total 147 Ktot 392 kpad 0 | none | slab_rows 147 | ws 0 | -
fwd n3 224x224 c8 k64 7x7 s2,2 p3,3 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 147,1,1 block 256 kps 13 tiles_n 1 tiles_total 147 Ktot 392 kpad 0 | none | slab_rows 147 | ws 0 | -
dgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 0: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 294,1,1 block 256 kps 18 tiles_n 1 tiles_total 294 Ktot 576 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 1: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 294,1,1 block 256 kps 24 tiles_n 1 tiles_total 294 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 2: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 294,1,1 block 256 kps 24 tiles_n 1 tiles_total 294 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e0 : phase 3: igemm_rows_kernel<128, 32, 4, 1, 8, false, false> grid 294,1,1 block 256 kps 32 tiles_n 1 tiles_total 294 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
wgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 4,1,70 block 256 kps 17 tiles_n 4 tiles_total 4 | wgrad_reduce_kernel grid 98 | ws 1756160 | -
fwd n3 56x56 c64 k64 3x3 s1,1 p1,1 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 37,1,2 block 256 kps 9 tiles_n 1 tiles_total 37 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows 256 | ws 1204224 | -
dgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 wt1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 37,1,2 block 256 kps 9 tiles_n 1 tiles_total 37 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1204224 | -
dgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 wt0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, false, true> grid 37,1,2 block 256 kps 9 tiles_n 1 tiles_total 37 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1204224 | -
wgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 5,1,18 block 256 kps 17 tiles_n 5 tiles_total 5 | wgrad_reduce_kernel grid 144 | ws 663552 | -
fwd n3 56x56 c64 k128 3x3 s2,2 p1,1 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 19,1,2 block 256 kps 9 tiles_n 1 tiles_total 19 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 602112 | -
dgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 0: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 10,1,1 block 256 kps 4 tiles_n 1 tiles_total 10 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 1: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 10,1,1 block 256 kps 8 tiles_n 1 tiles_total 10 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 2: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 10,1,1 block 256 kps 8 tiles_n 1 tiles_total 10 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e0 : phase 3: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 10,1,1 block 256 kps 16 tiles_n 1 tiles_total 10 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
pair n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e0 : apart
fwd n3 56x56 c64 k128 1x1 s2,2 p0,0 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 19,1,1 block 256 kps 2 tiles_n 1 tiles_total 19 Ktot 64 kpad 0 | none | slab_rows 19 | ws 0 | -
dgrad n3 56x56 c64 k128 1x1 s2,2 p0,0 wt1 e0 : phase 0: igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 10,1,1 block 256 kps 4 tiles_n 1 tiles_total 10 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | -
fwd n3 17x17 c128 k128 1x7 s1,1 p0,3 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 7,1,3 block 256 kps 10 tiles_n 1 tiles_total 7 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows 109 | ws 332928 | -
dgrad n3 17x17 c128 k128 1x7 s1,1 p0,3 wt1 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 7,1,3 block 256 kps 10 tiles_n 1 tiles_total 7 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows - | ws 332928 | -
fwd n3 17x17 c128 k192 7x1 s1,1 p3,0 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 12,1,3 block 256 kps 10 tiles_n 3 tiles_total 12 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 3,109 | slab_rows 109 | ws 499392 | -
dgrad n3 17x17 c128 k192 7x1 s1,1 p3,0 wt1 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 7,1,5 block 256 kps 9 tiles_n 1 tiles_total 7 Ktot 1344 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows - | ws 554880 | -
fwd n3 35x35 c288 k384 3x3 s2,2 p0,0 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 21,1,9 block 256 kps 9 tiles_n 3 tiles_total 21 Ktot 2592 kpad 0 | splitk_finalize_kernel<64> grid 6,109 | slab_rows 109 | ws 2996352 | -
dgrad n3 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 24,1,1 block 256 kps 48 tiles_n 3 tiles_total 24 Ktot 1536 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 24,1,1 block 256 kps 24 tiles_n 3 tiles_total 24 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 24,1,1 block 256 kps 24 tiles_n 3 tiles_total 24 Ktot 768 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 21,1,1 block 256 kps 12 tiles_n 3 tiles_total 21 Ktot 384 kpad 0 | none | slab_rows - | ws 0 | -
fwd n3 35x35 c48 k64 5x5 s1,1 p2,2 stap0 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 15,1,4 block 256 kps 10 tiles_n 1 tiles_total 15 Ktot 1200 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows 256 | ws 940800 | -
dgrad n3 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, true> grid 15,1,6 block 256 kps 9 tiles_n 1 tiles_total 15 Ktot 1600 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1058400 | -
fwd n3 56x56 c128 k128 1x1 s1,1 p0,0 stap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 74,1,1 block 256 kps 4 tiles_n 1 tiles_total 74 Ktot 128 kpad 0 | none | slab_rows 74 | ws 0 | -
pointwise n3 56x56 c128 k64 ldb128 tapmap1 e0 : igemm_rows_kernel<256, 64, 4, 1, 8, true, false> grid 37,1,1 block 256 kps 4 tiles_n 1 tiles_total 37 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | -
pointwise n3 1x1 c512 k1000 ldb512 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 8,1,2 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 512 kpad 0 | splitk_finalize_kernel<64> grid 16,1 | slab_rows - | ws 6000 | -
pointwise n3 1x1 c1000 k512 ldb512 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, false, true> grid 4,1,4 block 256 kps 8 tiles_n 4 tiles_total 4 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 8,1 | slab_rows - | ws 6144 | -
wgrad n3 1x1 c512 k1000 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 32,1,1 block 256 kps 1 tiles_n 4 tiles_total 32 | none | ws 0 | -
pointwise n3 1x1 c2048 k1000 ldb2048 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 8,1,8 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 2048 kpad 0 | splitk_finalize_kernel<64> grid 16,1 | slab_rows - | ws 24000 | -
pointwise n3 1x1 c1000 k2048 ldb2048 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, false, true> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,1 | slab_rows - | ws 24576 | -
pointwise n3 1x1 c1000 k2048 ldb1000 tapmap1 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, true> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,1 | slab_rows - | ws 24576 | -
wgrad n3 1x1 c2048 k1000 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 128,1,1 block 256 kps 1 tiles_n 16 tiles_total 128 | none | ws 0 | -
pointwise n3 1x1 c512 k64500 ldb512 tapmap0 e0 : igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 504,1,1 block 256 kps 16 tiles_n 504 tiles_total 504 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
pointwise n3 1x1 c64500 k512 ldb64500 tapmap1 e0 : igemm_rows_kernel<128, 128, 2, 2, 4, true, true> grid 4,1,63 block 256 kps 32 tiles_n 4 tiles_total 4 Ktot 64500 kpad 0 | splitk_finalize_kernel<64> grid 8,1 | slab_rows - | ws 96768 | -
wgrad n3 1x1 c512 k64500 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 4, 8> grid 2016,1,1 block 256 kps 1 tiles_n 4 tiles_total 2016 | none | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 5,1,1 block 256 kps 8 tiles_n 1 tiles_total 5 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 5,1,1 block 256 kps 16 tiles_n 1 tiles_total 5 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 5,1,1 block 256 kps 16 tiles_n 1 tiles_total 5 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 5,1,1 block 256 kps 32 tiles_n 1 tiles_total 5 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
pair n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e0 : apart
dgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 4,1,1 block 256 kps 16 tiles_n 2 tiles_total 4 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 4,1,1 block 256 kps 32 tiles_n 2 tiles_total 4 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 4,1,1 block 256 kps 32 tiles_n 2 tiles_total 4 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, true, false> grid 4,1,1 block 256 kps 64 tiles_n 2 tiles_total 4 Ktot 2048 kpad 0 | none | slab_rows - | ws 0 | -
pair n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e0 : apart
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 0: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 5,1,1 block 256 kps 8 tiles_n 1 tiles_total 5 Ktot 256 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 1: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 5,1,1 block 256 kps 16 tiles_n 1 tiles_total 5 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 2: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 5,1,1 block 256 kps 16 tiles_n 1 tiles_total 5 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e0 : phase 3: igemm_rows_kernel<128, 128, 2, 2, 8, false, false> grid 5,1,1 block 256 kps 32 tiles_n 1 tiles_total 5 Ktot 1024 kpad 0 | none | slab_rows - | ws 0 | -
bnred n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e0 : not available
bnred n3 56x56 c64 k64 1x1 s1,1 p0,0 wt1 e0 : not available
bnred n3 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e0 : not available
wgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 5,1,4 block 256 kps 19 tiles_n 5 tiles_total 5 | wgrad_reduce_kernel grid 288 | ws 294912 | -
wgrad n3 56x56 c64 k128 1x1 s2,2 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 1,1,4 block 256 kps 19 tiles_n 1 tiles_total 1 | wgrad_reduce_kernel grid 32 | ws 32768 | -
wgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 72,1,1 block 256 kps 5 tiles_n 18 tiles_total 72 | none | ws 0 | -
wgrad n3 14x14 c256 k512 1x1 s2,2 p0,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 8,1,1 block 256 kps 5 tiles_n 2 tiles_total 8 | none | ws 0 | -
wgrad n3 17x17 c128 k192 7x1 s1,1 p3,0 e0 : igemm_wgrad_kernel<128, 128, 2, 2, 8, 8> grid 14,1,1 block 256 kps 28 tiles_n 7 tiles_total 14 | none | ws 0 | -
wgrad n3 35x35 c48 k64 5x5 s1,1 p2,2 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 10,1,7 block 256 kps 17 tiles_n 10 tiles_total 10 | wgrad_reduce_kernel grid 300 | ws 537600 | -
wgrad n3 56x56 c256 k64 1x1 s1,1 p0,0 e0 : igemm_wgrad_kernel<64, 128, 2, 2, 8, 8> grid 2,1,18 block 256 kps 17 tiles_n 2 tiles_total 2 | wgrad_reduce_kernel grid 64 | ws 294912 | -
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 3136,1,1 block 256 kps 14 tiles_n 1 tiles_total 3136 Ktot 448 kpad 0 | none | slab_rows 3136 | ws 0 | rows10 M401408 N64 K448 a224x224x8 o112x112 U2,2 O-3,-3 T14 s1 b0 r0 p0
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 3136,1,1 block 256 kps 49 tiles_n 1 tiles_total 3136 Ktot 1568 kpad 1 | none | slab_rows 3136 | ws 0 | rows10 M401408 N64 K1568 a224x224x8 o112x112 U2,2 O-3,-3 T49 s0 b0 r0 p0
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e1 : igemm_rows_dma_uni_kernel<128, 32, 4, 1, false, false, true> grid 12544,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 12544 Ktot 0 kpad 0 ph 3136 3136 3136 3136 | none | slab_rows - | ws 0 | rows00 M0 N8 K0 a112x112x64 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 401408,576 401408,768 401408,768 401408,1024
wgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 4,1,128 block 256 kps 98 tiles_n 4 tiles_total 4 inc 64,0,224,224,512,1792,0 | wgrad_reduce_kernel grid 98 | ws 6422528 | wgrad K64 N392 P401408 x224x224x8 o112x112 f7x7 s2,2 p3,3
fwd n32 56x56 c64 k64 3x3 s1,1 p1,1 stap0 e1 : halo
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt1 e1 : halo
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, false, false, false> grid 784,1,1 block 256 kps 18 tiles_n 1 tiles_total 784 Ktot 576 kpad 0 | none | slab_rows - | ws 0 | rows00 M100352 N64 K576 a56x56x64 o56x56 U1,1 O0,0 T9 s0 b0 r0 p0
wgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 e1 : halo
fwd n32 56x56 c64 k128 3x3 s2,2 p1,1 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 196,1,2 block 256 kps 9 tiles_n 1 tiles_total 196 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 6422528 | rows11 M25088 N128 K576 a56x56x64 o28x28 U2,2 O-1,-1 T9 s0 b0 r0 p0
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 784,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 784 Ktot 0 kpad 0 ph 196 196 196 196 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 25088,128 25088,256 25088,256 25088,512
pair n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 784,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 784 Ktot 0 kpad 0 ph 196 196 196 196 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 25088,256 25088,256 25088,256 25088,512
fwd n32 56x56 c64 k128 1x1 s2,2 p0,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 196,1,1 block 256 kps 2 tiles_n 1 tiles_total 196 Ktot 64 kpad 0 | none | slab_rows 196 | ws 0 | rows10 M25088 N128 K64 a56x56x64 o28x28 U2,2 O0,0 T1 s0 b0 r0 p0
dgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 196 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p1 25088,128
fwd n32 17x17 c128 k128 1x7 s1,1 p0,3 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 73,1,3 block 256 kps 10 tiles_n 1 tiles_total 73 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 3551232 | rows11 M9248 N128 K896 a17x17x128 o17x17 U1,1 O0,-3 T7 s0 b0 r0 p0
dgrad n32 17x17 c128 k128 1x7 s1,1 p0,3 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 73,1,3 block 256 kps 10 tiles_n 1 tiles_total 73 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows - | ws 3551232 | rows11 M9248 N128 K896 a17x17x128 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n32 17x17 c128 k192 7x1 s1,1 p3,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, true, false> grid 219,1,3 block 256 kps 10 tiles_n 3 tiles_total 219 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 3,256 | slab_rows 256 | ws 5326848 | rows11 M9248 N192 K896 a17x17x128 o17x17 U1,1 O-3,0 T7 s0 b0 r0 p0
dgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 73,1,5 block 256 kps 9 tiles_n 1 tiles_total 73 Ktot 1344 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows - | ws 5918720 | rows11 M9248 N128 K1344 a17x17x192 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n32 35x35 c288 k384 3x3 s2,2 p0,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 219,1,3 block 256 kps 27 tiles_n 3 tiles_total 219 Ktot 2592 kpad 0 | splitk_finalize_kernel<64> grid 6,171 | slab_rows 171 | ws 10653696 | rows11 M9248 N384 K2592 a35x35x288 o17x17 U2,2 O0,0 T9 s0 b0 r0 p0
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 972,1,1 block 256 kps 1073741824 tiles_n 3 tiles_total 972 Ktot 0 kpad 0 ph 243 231 231 219 | none | slab_rows - | ws 0 | rows10 M0 N288 K0 a17x17x384 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 10368,1536 9792,768 9792,768 9248,384
fwd n32 35x35 c48 k64 5x5 s1,1 p2,2 stap0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 307,1,1 block 256 kps 50 tiles_n 1 tiles_total 307 Ktot 1600 kpad 1 | none | slab_rows 307 | ws 10035200 | rows10 M39200 N64 K1600 a35x35x48 o35x35 U1,1 O-2,-2 T25 s0 b0 r0 p0
dgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 307,1,1 block 256 kps 50 tiles_n 1 tiles_total 307 Ktot 1600 kpad 0 | none | slab_rows - | ws 7526400 | rows11 M39200 N48 K1600 a35x35x64 o35x35 U1,1 O0,0 T25 s0 b0 r0 p0
fwd n32 56x56 c128 k128 1x1 s1,1 p0,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 784,1,1 block 256 kps 4 tiles_n 1 tiles_total 784 Ktot 128 kpad 0 | none | slab_rows 784 | ws 0 | rows10 M100352 N128 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 56x56 c128 k64 ldb128 tapmap1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 784,1,1 block 256 kps 4 tiles_n 1 tiles_total 784 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | rows10 M100352 N64 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c512 k1000 ldb512 tapmap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,2 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 512 kpad 0 | splitk_finalize_kernel<64> grid 16,4 | slab_rows - | ws 64000 | rows11 M32 N1000 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c1000 k512 ldb512 tapmap0 e1 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 4,1,4 block 256 kps 8 tiles_n 4 tiles_total 4 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 8,4 | slab_rows - | ws 65536 | rows01 M32 N512 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n32 1x1 c512 k1000 1x1 s1,1 p0,0 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 16,1,1 block 512 kps 1 tiles_n 2 tiles_total 16 | none | ws 0 | wgrad K1000 N512 P32 x1x1x512 o1x1 f1x1 s1,1 p0,0
pointwise n32 1x1 c2048 k1000 ldb2048 tapmap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,8 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 2048 kpad 0 | splitk_finalize_kernel<64> grid 16,4 | slab_rows - | ws 256000 | rows11 M32 N1000 K2048 a1x1x2048 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c1000 k2048 ldb2048 tapmap0 e1 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,4 | slab_rows - | ws 262144 | rows01 M32 N2048 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c1000 k2048 ldb1000 tapmap1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 16,1,1 block 256 kps 32 tiles_n 16 tiles_total 16 Ktot 1024 kpad 1 | none | slab_rows - | ws 262144 | rows10 M32 N2048 K1024 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n32 1x1 c2048 k1000 1x1 s1,1 p0,0 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 64,1,1 block 512 kps 1 tiles_n 8 tiles_total 64 | none | ws 0 | wgrad K1000 N2048 P32 x1x1x2048 o1x1 f1x1 s1,1 p0,0
pointwise n32 1x1 c512 k64500 ldb512 tapmap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 504,1,1 block 256 kps 16 tiles_n 504 tiles_total 504 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | rows10 M32 N64500 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c64500 k512 ldb64500 tapmap1 e1 : igemm_rows_kernel<128, 128, 2, 2, 4, true, true> grid 4,1,63 block 256 kps 32 tiles_n 4 tiles_total 4 Ktot 64500 kpad 0 | splitk_finalize_kernel<64> grid 8,4 | slab_rows - | ws 1032192 | -
wgrad n32 1x1 c512 k64500 1x1 s1,1 p0,0 e1 : igemm_wgrad_kernel<128, 128, 2, 2, 4, 8> grid 2016,1,1 block 256 kps 1 tiles_n 4 tiles_total 2016 | none | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 6272,256 6272,512 6272,512 6272,1024
pair n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 6272,512 6272,512 6272,512 6272,1024
dgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 104,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 104 Ktot 0 kpad 0 ph 26 26 26 26 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 1568,512 1568,1024 1568,1024 1568,2048
pair n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 104,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 104 Ktot 0 kpad 0 ph 26 26 26 26 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 1568,1024 1568,1024 1568,1024 1568,2048
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, false, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows - | ws 0 | rows00 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 6272,256 6272,512 6272,512 6272,1024
bnred n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows 196 | ws 0
bnred n32 56x56 c64 k64 1x1 s1,1 p0,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 784,1,1 block 256 kps 2 tiles_n 1 tiles_total 784 Ktot 64 kpad 0 | none | slab_rows 784 | ws 0
bnred n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 307,1,1 block 256 kps 50 tiles_n 1 tiles_total 307 Ktot 1600 kpad 0 | none | slab_rows 307 | ws 0
wgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 e1 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 5,1,49 block 256 kps 16 tiles_n 5 tiles_total 5 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 288 | ws 3612672 | wgrad K128 N576 P25088 x56x56x64 o28x28 f3x3 s2,2 p1,1
wgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,49 block 256 kps 16 tiles_n 1 tiles_total 2 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 32 | ws 401408 | wgrad K128 N64 P25088 x56x56x64 o28x28 f1x1 s2,2 p0,0
wgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 36,1,3 block 512 kps 17 tiles_n 9 tiles_total 36 | wgrad_reduce_kernel grid 4608 | ws 3538944 | wgrad K512 N2304 P1568 x14x14x256 o7x7 f3x3 s2,2 p1,1
wgrad n32 14x14 c256 k512 1x1 s2,2 p0,0 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 4,1,3 block 512 kps 17 tiles_n 1 tiles_total 4 | wgrad_reduce_kernel grid 512 | ws 393216 | wgrad K512 N256 P1568 x14x14x256 o7x7 f1x1 s2,2 p0,0
wgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 e1 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 14,1,17 block 256 kps 17 tiles_n 7 tiles_total 14 inc 15,1,17,17,4096,0,0 | wgrad_reduce_kernel grid 672 | ws 2924544 | wgrad K192 N896 P9248 x17x17x128 o17x17 f7x1 s1,1 p3,0
wgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 10,1,52 block 256 kps 24 tiles_n 10 tiles_total 10 inc 32,0,35,35,1536,0,0 | wgrad_reduce_kernel grid 300 | ws 5606400 | wgrad K64 N1200 P39200 x35x35x48 o35x35 f5x5 s1,1 p2,2
wgrad n32 56x56 c256 k64 1x1 s1,1 p0,0 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,196 block 256 kps 16 tiles_n 2 tiles_total 2 inc 32,0,56,56,8192,0,0 | wgrad_reduce_kernel grid 64 | ws 3211264 | wgrad K64 N256 P100352 x56x56x256 o56x56 f1x1 s1,1 p0,0
fwd n3 224x224 c8 k64 7x7 s2,2 p3,3 stap1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 294,1,1 block 256 kps 14 tiles_n 1 tiles_total 294 Ktot 448 kpad 0 | none | slab_rows 294 | ws 0 | rows10 M37632 N64 K448 a224x224x8 o112x112 U2,2 O-3,-3 T14 s1 b0 r0 p0
fwd n3 224x224 c8 k64 7x7 s2,2 p3,3 stap0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 294,1,1 block 256 kps 49 tiles_n 1 tiles_total 294 Ktot 1568 kpad 1 | none | slab_rows 294 | ws 0 | rows10 M37632 N64 K1568 a224x224x8 o112x112 U2,2 O-3,-3 T49 s0 b0 r0 p0
dgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e1 : igemm_rows_dma_uni_kernel<128, 32, 4, 1, false, false, true> grid 1176,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 1176 Ktot 0 kpad 0 ph 294 294 294 294 | none | slab_rows - | ws 0 | rows00 M0 N8 K0 a112x112x64 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 37632,576 37632,768 37632,768 37632,1024
wgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 4,1,70 block 256 kps 17 tiles_n 4 tiles_total 4 inc 64,0,224,224,512,1792,0 | wgrad_reduce_kernel grid 98 | ws 1756160 | wgrad K64 N392 P37632 x224x224x8 o112x112 f7x7 s2,2 p3,3
fwd n3 56x56 c64 k64 3x3 s1,1 p1,1 stap0 e1 : halo
dgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 wt1 e1 : halo
dgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 wt0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, false, true, false> grid 74,1,2 block 256 kps 9 tiles_n 1 tiles_total 74 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1204224 | rows01 M9408 N64 K576 a56x56x64 o56x56 U1,1 O0,0 T9 s0 b0 r0 p0
wgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 e1 : halo
fwd n3 56x56 c64 k128 3x3 s2,2 p1,1 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 19,1,2 block 256 kps 9 tiles_n 1 tiles_total 19 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 602112 | rows11 M2352 N128 K576 a56x56x64 o28x28 U2,2 O-1,-1 T9 s0 b0 r0 p0
dgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 76,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 76 Ktot 0 kpad 0 ph 19 19 19 19 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 2352,128 2352,256 2352,256 2352,512
pair n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 76,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 76 Ktot 0 kpad 0 ph 19 19 19 19 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 2352,256 2352,256 2352,256 2352,512
fwd n3 56x56 c64 k128 1x1 s2,2 p0,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 19,1,1 block 256 kps 2 tiles_n 1 tiles_total 19 Ktot 64 kpad 0 | none | slab_rows 19 | ws 0 | rows10 M2352 N128 K64 a56x56x64 o28x28 U2,2 O0,0 T1 s0 b0 r0 p0
dgrad n3 56x56 c64 k128 1x1 s2,2 p0,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 19,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 19 Ktot 0 kpad 0 ph 19 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p1 2352,128
fwd n3 17x17 c128 k128 1x7 s1,1 p0,3 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 7,1,3 block 256 kps 10 tiles_n 1 tiles_total 7 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows 109 | ws 332928 | rows11 M867 N128 K896 a17x17x128 o17x17 U1,1 O0,-3 T7 s0 b0 r0 p0
dgrad n3 17x17 c128 k128 1x7 s1,1 p0,3 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 7,1,3 block 256 kps 10 tiles_n 1 tiles_total 7 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows - | ws 332928 | rows11 M867 N128 K896 a17x17x128 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n3 17x17 c128 k192 7x1 s1,1 p3,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, true, false> grid 21,1,3 block 256 kps 10 tiles_n 3 tiles_total 21 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 3,109 | slab_rows 109 | ws 499392 | rows11 M867 N192 K896 a17x17x128 o17x17 U1,1 O-3,0 T7 s0 b0 r0 p0
dgrad n3 17x17 c128 k192 7x1 s1,1 p3,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 7,1,5 block 256 kps 9 tiles_n 1 tiles_total 7 Ktot 1344 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows - | ws 554880 | rows11 M867 N128 K1344 a17x17x192 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n3 35x35 c288 k384 3x3 s2,2 p0,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 21,1,9 block 256 kps 9 tiles_n 3 tiles_total 21 Ktot 2592 kpad 0 | splitk_finalize_kernel<64> grid 6,109 | slab_rows 109 | ws 2996352 | rows11 M867 N384 K2592 a35x35x288 o17x17 U2,2 O0,0 T9 s0 b0 r0 p0
dgrad n3 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 96,1,1 block 256 kps 1073741824 tiles_n 3 tiles_total 96 Ktot 0 kpad 0 ph 24 24 24 21 | none | slab_rows - | ws 0 | rows10 M0 N288 K0 a17x17x384 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 972,1536 918,768 918,768 867,384
fwd n3 35x35 c48 k64 5x5 s1,1 p2,2 stap0 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 29,1,1 block 256 kps 50 tiles_n 1 tiles_total 29 Ktot 1600 kpad 1 | none | slab_rows 29 | ws 940800 | rows10 M3675 N64 K1600 a35x35x48 o35x35 U1,1 O-2,-2 T25 s0 b0 r0 p0
dgrad n3 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, true, false> grid 29,1,6 block 256 kps 9 tiles_n 1 tiles_total 29 Ktot 1600 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1058400 | rows11 M3675 N48 K1600 a35x35x64 o35x35 U1,1 O0,0 T25 s0 b0 r0 p0
fwd n3 56x56 c128 k128 1x1 s1,1 p0,0 stap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 74,1,1 block 256 kps 4 tiles_n 1 tiles_total 74 Ktot 128 kpad 0 | none | slab_rows 74 | ws 0 | rows10 M9408 N128 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 56x56 c128 k64 ldb128 tapmap1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 74,1,1 block 256 kps 4 tiles_n 1 tiles_total 74 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | rows10 M9408 N64 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c512 k1000 ldb512 tapmap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,2 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 512 kpad 0 | splitk_finalize_kernel<64> grid 16,1 | slab_rows - | ws 6000 | rows11 M3 N1000 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c1000 k512 ldb512 tapmap0 e1 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 4,1,4 block 256 kps 8 tiles_n 4 tiles_total 4 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 8,1 | slab_rows - | ws 6144 | rows01 M3 N512 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n3 1x1 c512 k1000 1x1 s1,1 p0,0 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 16,1,1 block 512 kps 1 tiles_n 2 tiles_total 16 | none | ws 0 | wgrad K1000 N512 P3 x1x1x512 o1x1 f1x1 s1,1 p0,0
pointwise n3 1x1 c2048 k1000 ldb2048 tapmap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,8 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 2048 kpad 0 | splitk_finalize_kernel<64> grid 16,1 | slab_rows - | ws 24000 | rows11 M3 N1000 K2048 a1x1x2048 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c1000 k2048 ldb2048 tapmap0 e1 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,1 | slab_rows - | ws 24576 | rows01 M3 N2048 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c1000 k2048 ldb1000 tapmap1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 16,1,1 block 256 kps 32 tiles_n 16 tiles_total 16 Ktot 1024 kpad 1 | none | slab_rows - | ws 24576 | rows10 M3 N2048 K1024 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n3 1x1 c2048 k1000 1x1 s1,1 p0,0 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 64,1,1 block 512 kps 1 tiles_n 8 tiles_total 64 | none | ws 0 | wgrad K1000 N2048 P3 x1x1x2048 o1x1 f1x1 s1,1 p0,0
pointwise n3 1x1 c512 k64500 ldb512 tapmap0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 504,1,1 block 256 kps 16 tiles_n 504 tiles_total 504 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | rows10 M3 N64500 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c64500 k512 ldb64500 tapmap1 e1 : igemm_rows_kernel<128, 128, 2, 2, 4, true, true> grid 4,1,63 block 256 kps 32 tiles_n 4 tiles_total 4 Ktot 64500 kpad 0 | splitk_finalize_kernel<64> grid 8,1 | slab_rows - | ws 96768 | -
wgrad n3 1x1 c512 k64500 1x1 s1,1 p0,0 e1 : igemm_wgrad_kernel<128, 128, 2, 2, 4, 8> grid 2016,1,1 block 256 kps 1 tiles_n 4 tiles_total 2016 | none | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 588,256 588,512 588,512 588,1024
pair n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 588,512 588,512 588,512 588,1024
dgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 16,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 16 Ktot 0 kpad 0 ph 4 4 4 4 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 147,512 147,1024 147,1024 147,2048
pair n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 16,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 16 Ktot 0 kpad 0 ph 4 4 4 4 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 147,1024 147,1024 147,1024 147,2048
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, false, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows - | ws 0 | rows00 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 588,256 588,512 588,512 588,1024
bnred n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e1 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows 20 | ws 0
bnred n3 56x56 c64 k64 1x1 s1,1 p0,0 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 74,1,1 block 256 kps 2 tiles_n 1 tiles_total 74 Ktot 64 kpad 0 | none | slab_rows 74 | ws 0
bnred n3 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e1 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 29,1,1 block 256 kps 50 tiles_n 1 tiles_total 29 Ktot 1600 kpad 0 | none | slab_rows 29 | ws 0
wgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 e1 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 5,1,4 block 256 kps 19 tiles_n 5 tiles_total 5 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 288 | ws 294912 | wgrad K128 N576 P2352 x56x56x64 o28x28 f3x3 s2,2 p1,1
wgrad n3 56x56 c64 k128 1x1 s2,2 p0,0 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,4 block 256 kps 19 tiles_n 1 tiles_total 2 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 32 | ws 32768 | wgrad K128 N64 P2352 x56x56x64 o28x28 f1x1 s2,2 p0,0
wgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 36,1,1 block 512 kps 5 tiles_n 9 tiles_total 36 | none | ws 0 | wgrad K512 N2304 P147 x14x14x256 o7x7 f3x3 s2,2 p1,1
wgrad n3 14x14 c256 k512 1x1 s2,2 p0,0 e1 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 4,1,1 block 512 kps 5 tiles_n 1 tiles_total 4 | none | ws 0 | wgrad K512 N256 P147 x14x14x256 o7x7 f1x1 s2,2 p0,0
wgrad n3 17x17 c128 k192 7x1 s1,1 p3,0 e1 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 14,1,1 block 256 kps 28 tiles_n 7 tiles_total 14 inc 15,1,17,17,4096,0,0 | none | ws 0 | wgrad K192 N896 P867 x17x17x128 o17x17 f7x1 s1,1 p3,0
wgrad n3 35x35 c48 k64 5x5 s1,1 p2,2 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 10,1,7 block 256 kps 17 tiles_n 10 tiles_total 10 inc 32,0,35,35,1536,0,0 | wgrad_reduce_kernel grid 300 | ws 537600 | wgrad K64 N1200 P3675 x35x35x48 o35x35 f5x5 s1,1 p2,2
wgrad n3 56x56 c256 k64 1x1 s1,1 p0,0 e1 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,18 block 256 kps 17 tiles_n 2 tiles_total 2 inc 32,0,56,56,8192,0,0 | wgrad_reduce_kernel grid 64 | ws 294912 | wgrad K64 N256 P9408 x56x56x256 o56x56 f1x1 s1,1 p0,0
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 3136,1,1 block 256 kps 14 tiles_n 1 tiles_total 3136 Ktot 448 kpad 0 | none | slab_rows 3136 | ws 0 | rows10 M401408 N64 K448 a224x224x8 o112x112 U2,2 O-3,-3 T14 s1 b0 r0 p0
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 3136,1,1 block 256 kps 49 tiles_n 1 tiles_total 3136 Ktot 1568 kpad 1 | none | slab_rows 3136 | ws 0 | rows10 M401408 N64 K1568 a224x224x8 o112x112 U2,2 O-3,-3 T49 s0 b0 r0 p0
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e2 : igemm_rows_dma_uni_kernel<128, 32, 4, 1, false, false, true> grid 12544,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 12544 Ktot 0 kpad 0 ph 3136 3136 3136 3136 | none | slab_rows - | ws 0 | rows00 M0 N8 K0 a112x112x64 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 401408,576 401408,768 401408,768 401408,1024
wgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 4,1,128 block 256 kps 98 tiles_n 4 tiles_total 4 inc 64,0,224,224,512,1792,0 | wgrad_reduce_kernel grid 98 | ws 6422528 | wgrad K64 N392 P401408 x224x224x8 o112x112 f7x7 s2,2 p3,3
fwd n32 56x56 c64 k64 3x3 s1,1 p1,1 stap0 e2 : halo
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt1 e2 : halo
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, false, false, false> grid 784,1,1 block 256 kps 18 tiles_n 1 tiles_total 784 Ktot 576 kpad 0 | none | slab_rows - | ws 0 | rows00 M100352 N64 K576 a56x56x64 o56x56 U1,1 O0,0 T9 s0 b0 r0 p0
wgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 e2 : halo
fwd n32 56x56 c64 k128 3x3 s2,2 p1,1 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 196,1,2 block 256 kps 9 tiles_n 1 tiles_total 196 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 6422528 | rows11 M25088 N128 K576 a56x56x64 o28x28 U2,2 O-1,-1 T9 s0 b0 r0 p0
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 784,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 784 Ktot 0 kpad 0 ph 196 196 196 196 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 25088,128 25088,256 25088,256 25088,512
pair n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 784,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 784 Ktot 0 kpad 0 ph 196 196 196 196 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 25088,256 25088,256 25088,256 25088,512
fwd n32 56x56 c64 k128 1x1 s2,2 p0,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 196,1,1 block 256 kps 2 tiles_n 1 tiles_total 196 Ktot 64 kpad 0 | none | slab_rows 196 | ws 0 | rows10 M25088 N128 K64 a56x56x64 o28x28 U2,2 O0,0 T1 s0 b0 r0 p0
dgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 196 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p1 25088,128
fwd n32 17x17 c128 k128 1x7 s1,1 p0,3 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 73,1,3 block 256 kps 10 tiles_n 1 tiles_total 73 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 3551232 | rows11 M9248 N128 K896 a17x17x128 o17x17 U1,1 O0,-3 T7 s0 b0 r0 p0
dgrad n32 17x17 c128 k128 1x7 s1,1 p0,3 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 73,1,3 block 256 kps 10 tiles_n 1 tiles_total 73 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows - | ws 3551232 | rows11 M9248 N128 K896 a17x17x128 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n32 17x17 c128 k192 7x1 s1,1 p3,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, true, false> grid 219,1,3 block 256 kps 10 tiles_n 3 tiles_total 219 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 3,256 | slab_rows 256 | ws 5326848 | rows11 M9248 N192 K896 a17x17x128 o17x17 U1,1 O-3,0 T7 s0 b0 r0 p0
dgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 73,1,5 block 256 kps 9 tiles_n 1 tiles_total 73 Ktot 1344 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows - | ws 5918720 | rows11 M9248 N128 K1344 a17x17x192 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n32 35x35 c288 k384 3x3 s2,2 p0,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 219,1,3 block 256 kps 27 tiles_n 3 tiles_total 219 Ktot 2592 kpad 0 | splitk_finalize_kernel<64> grid 6,171 | slab_rows 171 | ws 10653696 | rows11 M9248 N384 K2592 a35x35x288 o17x17 U2,2 O0,0 T9 s0 b0 r0 p0
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 972,1,1 block 256 kps 1073741824 tiles_n 3 tiles_total 972 Ktot 0 kpad 0 ph 243 231 231 219 | none | slab_rows - | ws 0 | rows10 M0 N288 K0 a17x17x384 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 10368,1536 9792,768 9792,768 9248,384
fwd n32 35x35 c48 k64 5x5 s1,1 p2,2 stap0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 307,1,1 block 256 kps 50 tiles_n 1 tiles_total 307 Ktot 1600 kpad 1 | none | slab_rows 307 | ws 10035200 | rows10 M39200 N64 K1600 a35x35x48 o35x35 U1,1 O-2,-2 T25 s0 b0 r0 p0
dgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 307,1,1 block 256 kps 50 tiles_n 1 tiles_total 307 Ktot 1600 kpad 0 | none | slab_rows - | ws 7526400 | rows11 M39200 N48 K1600 a35x35x64 o35x35 U1,1 O0,0 T25 s0 b0 r0 p0
fwd n32 56x56 c128 k128 1x1 s1,1 p0,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 784,1,1 block 256 kps 4 tiles_n 1 tiles_total 784 Ktot 128 kpad 0 | none | slab_rows 784 | ws 0 | rows10 M100352 N128 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 56x56 c128 k64 ldb128 tapmap1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 784,1,1 block 256 kps 4 tiles_n 1 tiles_total 784 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | rows10 M100352 N64 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c512 k1000 ldb512 tapmap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,2 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 512 kpad 0 | splitk_finalize_kernel<64> grid 16,4 | slab_rows - | ws 64000 | rows11 M32 N1000 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c1000 k512 ldb512 tapmap0 e2 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 4,1,4 block 256 kps 8 tiles_n 4 tiles_total 4 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 8,4 | slab_rows - | ws 65536 | rows01 M32 N512 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n32 1x1 c512 k1000 1x1 s1,1 p0,0 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 16,1,1 block 512 kps 1 tiles_n 2 tiles_total 16 | none | ws 0 | wgrad K1000 N512 P32 x1x1x512 o1x1 f1x1 s1,1 p0,0
pointwise n32 1x1 c2048 k1000 ldb2048 tapmap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,8 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 2048 kpad 0 | splitk_finalize_kernel<64> grid 16,4 | slab_rows - | ws 256000 | rows11 M32 N1000 K2048 a1x1x2048 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c1000 k2048 ldb2048 tapmap0 e2 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,4 | slab_rows - | ws 262144 | rows01 M32 N2048 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c1000 k2048 ldb1000 tapmap1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 16,1,1 block 256 kps 32 tiles_n 16 tiles_total 16 Ktot 1024 kpad 1 | none | slab_rows - | ws 262144 | rows10 M32 N2048 K1024 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n32 1x1 c2048 k1000 1x1 s1,1 p0,0 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 64,1,1 block 512 kps 1 tiles_n 8 tiles_total 64 | none | ws 0 | wgrad K1000 N2048 P32 x1x1x2048 o1x1 f1x1 s1,1 p0,0
pointwise n32 1x1 c512 k64500 ldb512 tapmap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 504,1,1 block 256 kps 16 tiles_n 504 tiles_total 504 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | rows10 M32 N64500 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n32 1x1 c64500 k512 ldb64500 tapmap1 e2 : igemm_rows_kernel<128, 128, 2, 2, 4, true, true> grid 4,1,63 block 256 kps 32 tiles_n 4 tiles_total 4 Ktot 64500 kpad 0 | splitk_finalize_kernel<64> grid 8,4 | slab_rows - | ws 1032192 | -
wgrad n32 1x1 c512 k64500 1x1 s1,1 p0,0 e2 : igemm_wgrad_kernel<128, 128, 2, 2, 4, 8> grid 2016,1,1 block 256 kps 1 tiles_n 4 tiles_total 2016 | none | ws 0 | -
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 6272,256 6272,512 6272,512 6272,1024
pair n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 6272,512 6272,512 6272,512 6272,1024
dgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 104,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 104 Ktot 0 kpad 0 ph 26 26 26 26 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 1568,512 1568,1024 1568,1024 1568,2048
pair n32 14x14 c256 k512 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 104,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 104 Ktot 0 kpad 0 ph 26 26 26 26 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 1568,1024 1568,1024 1568,1024 1568,2048
dgrad n32 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, false, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows - | ws 0 | rows00 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 6272,256 6272,512 6272,512 6272,1024
bnred n32 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 196,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 196 Ktot 0 kpad 0 ph 49 49 49 49 | none | slab_rows 196 | ws 0
bnred n32 56x56 c64 k64 1x1 s1,1 p0,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 784,1,1 block 256 kps 2 tiles_n 1 tiles_total 784 Ktot 64 kpad 0 | none | slab_rows 784 | ws 0
bnred n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 307,1,1 block 256 kps 50 tiles_n 1 tiles_total 307 Ktot 1600 kpad 0 | none | slab_rows 307 | ws 0
wgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 e2 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 5,1,49 block 256 kps 16 tiles_n 5 tiles_total 5 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 288 | ws 3612672 | wgrad K128 N576 P25088 x56x56x64 o28x28 f3x3 s2,2 p1,1
wgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,49 block 256 kps 16 tiles_n 1 tiles_total 2 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 32 | ws 401408 | wgrad K128 N64 P25088 x56x56x64 o28x28 f1x1 s2,2 p0,0
wgrad n32 14x14 c256 k512 3x3 s2,2 p1,1 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 36,1,3 block 512 kps 17 tiles_n 9 tiles_total 36 | wgrad_reduce_kernel grid 4608 | ws 3538944 | wgrad K512 N2304 P1568 x14x14x256 o7x7 f3x3 s2,2 p1,1
wgrad n32 14x14 c256 k512 1x1 s2,2 p0,0 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 4,1,3 block 512 kps 17 tiles_n 1 tiles_total 4 | wgrad_reduce_kernel grid 512 | ws 393216 | wgrad K512 N256 P1568 x14x14x256 o7x7 f1x1 s2,2 p0,0
wgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 e2 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 14,1,17 block 256 kps 17 tiles_n 7 tiles_total 14 inc 15,1,17,17,4096,0,0 | wgrad_reduce_kernel grid 672 | ws 2924544 | wgrad K192 N896 P9248 x17x17x128 o17x17 f7x1 s1,1 p3,0
wgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 10,1,52 block 256 kps 24 tiles_n 10 tiles_total 10 inc 32,0,35,35,1536,0,0 | wgrad_reduce_kernel grid 300 | ws 5606400 | wgrad K64 N1200 P39200 x35x35x48 o35x35 f5x5 s1,1 p2,2
wgrad n32 56x56 c256 k64 1x1 s1,1 p0,0 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,196 block 256 kps 16 tiles_n 2 tiles_total 2 inc 32,0,56,56,8192,0,0 | wgrad_reduce_kernel grid 64 | ws 3211264 | wgrad K64 N256 P100352 x56x56x256 o56x56 f1x1 s1,1 p0,0
fwd n3 224x224 c8 k64 7x7 s2,2 p3,3 stap1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 294,1,1 block 256 kps 14 tiles_n 1 tiles_total 294 Ktot 448 kpad 0 | none | slab_rows 294 | ws 0 | rows10 M37632 N64 K448 a224x224x8 o112x112 U2,2 O-3,-3 T14 s1 b0 r0 p0
fwd n3 224x224 c8 k64 7x7 s2,2 p3,3 stap0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 294,1,1 block 256 kps 49 tiles_n 1 tiles_total 294 Ktot 1568 kpad 1 | none | slab_rows 294 | ws 0 | rows10 M37632 N64 K1568 a224x224x8 o112x112 U2,2 O-3,-3 T49 s0 b0 r0 p0
dgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 wt0 e2 : igemm_rows_dma_uni_kernel<128, 32, 4, 1, false, false, true> grid 1176,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 1176 Ktot 0 kpad 0 ph 294 294 294 294 | none | slab_rows - | ws 0 | rows00 M0 N8 K0 a112x112x64 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 37632,576 37632,768 37632,768 37632,1024
wgrad n3 224x224 c8 k64 7x7 s2,2 p3,3 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 4,1,70 block 256 kps 17 tiles_n 4 tiles_total 4 inc 64,0,224,224,512,1792,0 | wgrad_reduce_kernel grid 98 | ws 1756160 | wgrad K64 N392 P37632 x224x224x8 o112x112 f7x7 s2,2 p3,3
fwd n3 56x56 c64 k64 3x3 s1,1 p1,1 stap0 e2 : halo
dgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 wt1 e2 : halo
dgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 wt0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, false, true, false> grid 74,1,2 block 256 kps 9 tiles_n 1 tiles_total 74 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1204224 | rows01 M9408 N64 K576 a56x56x64 o56x56 U1,1 O0,0 T9 s0 b0 r0 p0
wgrad n3 56x56 c64 k64 3x3 s1,1 p1,1 e2 : halo
fwd n3 56x56 c64 k128 3x3 s2,2 p1,1 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 19,1,2 block 256 kps 9 tiles_n 1 tiles_total 19 Ktot 576 kpad 0 | splitk_finalize_kernel<64> grid 2,256 | slab_rows 256 | ws 602112 | rows11 M2352 N128 K576 a56x56x64 o28x28 U2,2 O-1,-1 T9 s0 b0 r0 p0
dgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 76,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 76 Ktot 0 kpad 0 ph 19 19 19 19 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 2352,128 2352,256 2352,256 2352,512
pair n3 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 76,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 76 Ktot 0 kpad 0 ph 19 19 19 19 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 2352,256 2352,256 2352,256 2352,512
fwd n3 56x56 c64 k128 1x1 s2,2 p0,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 19,1,1 block 256 kps 2 tiles_n 1 tiles_total 19 Ktot 64 kpad 0 | none | slab_rows 19 | ws 0 | rows10 M2352 N128 K64 a56x56x64 o28x28 U2,2 O0,0 T1 s0 b0 r0 p0
dgrad n3 56x56 c64 k128 1x1 s2,2 p0,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, true> grid 19,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 19 Ktot 0 kpad 0 ph 19 | none | slab_rows - | ws 0 | rows10 M0 N64 K0 a28x28x128 o0x0 U1,1 O0,0 T0 s0 b0 r0 p1 2352,128
fwd n3 17x17 c128 k128 1x7 s1,1 p0,3 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 7,1,3 block 256 kps 10 tiles_n 1 tiles_total 7 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows 109 | ws 332928 | rows11 M867 N128 K896 a17x17x128 o17x17 U1,1 O0,-3 T7 s0 b0 r0 p0
dgrad n3 17x17 c128 k128 1x7 s1,1 p0,3 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 7,1,3 block 256 kps 10 tiles_n 1 tiles_total 7 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows - | ws 332928 | rows11 M867 N128 K896 a17x17x128 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n3 17x17 c128 k192 7x1 s1,1 p3,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, true, false> grid 21,1,3 block 256 kps 10 tiles_n 3 tiles_total 21 Ktot 896 kpad 0 | splitk_finalize_kernel<64> grid 3,109 | slab_rows 109 | ws 499392 | rows11 M867 N192 K896 a17x17x128 o17x17 U1,1 O-3,0 T7 s0 b0 r0 p0
dgrad n3 17x17 c128 k192 7x1 s1,1 p3,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 7,1,5 block 256 kps 9 tiles_n 1 tiles_total 7 Ktot 1344 kpad 0 | splitk_finalize_kernel<64> grid 2,109 | slab_rows - | ws 554880 | rows11 M867 N128 K1344 a17x17x192 o17x17 U1,1 O0,0 T7 s0 b0 r0 p0
fwd n3 35x35 c288 k384 3x3 s2,2 p0,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 21,1,9 block 256 kps 9 tiles_n 3 tiles_total 21 Ktot 2592 kpad 0 | splitk_finalize_kernel<64> grid 6,109 | slab_rows 109 | ws 2996352 | rows11 M867 N384 K2592 a35x35x288 o17x17 U2,2 O0,0 T9 s0 b0 r0 p0
dgrad n3 35x35 c288 k384 3x3 s2,2 p0,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 96,1,1 block 256 kps 1073741824 tiles_n 3 tiles_total 96 Ktot 0 kpad 0 ph 24 24 24 21 | none | slab_rows - | ws 0 | rows10 M0 N288 K0 a17x17x384 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 972,1536 918,768 918,768 867,384
fwd n3 35x35 c48 k64 5x5 s1,1 p2,2 stap0 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 29,1,1 block 256 kps 50 tiles_n 1 tiles_total 29 Ktot 1600 kpad 1 | none | slab_rows 29 | ws 940800 | rows10 M3675 N64 K1600 a35x35x48 o35x35 U1,1 O-2,-2 T25 s0 b0 r0 p0
dgrad n3 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, true, false> grid 29,1,6 block 256 kps 9 tiles_n 1 tiles_total 29 Ktot 1600 kpad 0 | splitk_finalize_kernel<64> grid 1,256 | slab_rows - | ws 1058400 | rows11 M3675 N48 K1600 a35x35x64 o35x35 U1,1 O0,0 T25 s0 b0 r0 p0
fwd n3 56x56 c128 k128 1x1 s1,1 p0,0 stap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 74,1,1 block 256 kps 4 tiles_n 1 tiles_total 74 Ktot 128 kpad 0 | none | slab_rows 74 | ws 0 | rows10 M9408 N128 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 56x56 c128 k64 ldb128 tapmap1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 74,1,1 block 256 kps 4 tiles_n 1 tiles_total 74 Ktot 128 kpad 0 | none | slab_rows - | ws 0 | rows10 M9408 N64 K128 a56x56x128 o56x56 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c512 k1000 ldb512 tapmap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,2 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 512 kpad 0 | splitk_finalize_kernel<64> grid 16,1 | slab_rows - | ws 6000 | rows11 M3 N1000 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c1000 k512 ldb512 tapmap0 e2 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 4,1,4 block 256 kps 8 tiles_n 4 tiles_total 4 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 8,1 | slab_rows - | ws 6144 | rows01 M3 N512 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n3 1x1 c512 k1000 1x1 s1,1 p0,0 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 16,1,1 block 512 kps 1 tiles_n 2 tiles_total 16 | none | ws 0 | wgrad K1000 N512 P3 x1x1x512 o1x1 f1x1 s1,1 p0,0
pointwise n3 1x1 c2048 k1000 ldb2048 tapmap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, true, false> grid 8,1,8 block 256 kps 8 tiles_n 8 tiles_total 8 Ktot 2048 kpad 0 | splitk_finalize_kernel<64> grid 16,1 | slab_rows - | ws 24000 | rows11 M3 N1000 K2048 a1x1x2048 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c1000 k2048 ldb2048 tapmap0 e2 : igemm_rows_dma_kernel<128, 128, 2, 2, false, true, false> grid 16,1,4 block 256 kps 8 tiles_n 16 tiles_total 16 Ktot 1000 kpad 0 | splitk_finalize_kernel<64> grid 32,1 | slab_rows - | ws 24576 | rows01 M3 N2048 K1000 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c1000 k2048 ldb1000 tapmap1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 16,1,1 block 256 kps 32 tiles_n 16 tiles_total 16 Ktot 1024 kpad 1 | none | slab_rows - | ws 24576 | rows10 M3 N2048 K1024 a1x1x1000 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
wgrad n3 1x1 c2048 k1000 1x1 s1,1 p0,0 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 64,1,1 block 512 kps 1 tiles_n 8 tiles_total 64 | none | ws 0 | wgrad K1000 N2048 P3 x1x1x2048 o1x1 f1x1 s1,1 p0,0
pointwise n3 1x1 c512 k64500 ldb512 tapmap0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, false> grid 504,1,1 block 256 kps 16 tiles_n 504 tiles_total 504 Ktot 512 kpad 0 | none | slab_rows - | ws 0 | rows10 M3 N64500 K512 a1x1x512 o1x1 U1,1 O0,0 T1 s0 b0 r0 p0
pointwise n3 1x1 c64500 k512 ldb64500 tapmap1 e2 : igemm_rows_kernel<128, 128, 2, 2, 4, true, true> grid 4,1,63 block 256 kps 32 tiles_n 4 tiles_total 4 Ktot 64500 kpad 0 | splitk_finalize_kernel<64> grid 8,1 | slab_rows - | ws 96768 | -
wgrad n3 1x1 c512 k64500 1x1 s1,1 p0,0 e2 : igemm_wgrad_kernel<128, 128, 2, 2, 4, 8> grid 2016,1,1 block 256 kps 1 tiles_n 4 tiles_total 2016 | none | ws 0 | -
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 588,256 588,512 588,512 588,1024
pair n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows - | ws 0 | rows10 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 588,512 588,512 588,512 588,1024
dgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 16,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 16 Ktot 0 kpad 0 ph 4 4 4 4 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 147,512 147,1024 147,1024 147,2048
pair n3 14x14 c256 k512 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 16,1,1 block 256 kps 1073741824 tiles_n 2 tiles_total 16 Ktot 0 kpad 0 ph 4 4 4 4 | none | slab_rows - | ws 0 | rows10 M0 N256 K0 a7x7x512 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 147,1024 147,1024 147,1024 147,2048
dgrad n3 28x28 c128 k256 3x3 s2,2 p1,1 wt0 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, false, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows - | ws 0 | rows00 M0 N128 K0 a14x14x256 o0x0 U1,1 O0,0 T0 s0 b0 r0 p4 588,256 588,512 588,512 588,1024
bnred n3 28x28 c128 k256 3x3 s2,2 p1,1 wt1 e2 : igemm_rows_dma_uni_kernel<128, 128, 2, 2, true, false, true> grid 20,1,1 block 256 kps 1073741824 tiles_n 1 tiles_total 20 Ktot 0 kpad 0 ph 5 5 5 5 | none | slab_rows 20 | ws 0
bnred n3 56x56 c64 k64 1x1 s1,1 p0,0 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 74,1,1 block 256 kps 2 tiles_n 1 tiles_total 74 Ktot 64 kpad 0 | none | slab_rows 74 | ws 0
bnred n3 35x35 c48 k64 5x5 s1,1 p2,2 wt1 e2 : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> grid 29,1,1 block 256 kps 50 tiles_n 1 tiles_total 29 Ktot 1600 kpad 0 | none | slab_rows 29 | ws 0
wgrad n3 56x56 c64 k128 3x3 s2,2 p1,1 e2 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 5,1,4 block 256 kps 19 tiles_n 5 tiles_total 5 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 288 | ws 294912 | wgrad K128 N576 P2352 x56x56x64 o28x28 f3x3 s2,2 p1,1
wgrad n3 56x56 c64 k128 1x1 s2,2 p0,0 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,4 block 256 kps 19 tiles_n 1 tiles_total 2 inc 8,2,56,56,7680,3584,0 | wgrad_reduce_kernel grid 32 | ws 32768 | wgrad K128 N64 P2352 x56x56x64 o28x28 f1x1 s2,2 p0,0
wgrad n3 14x14 c256 k512 3x3 s2,2 p1,1 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 36,1,1 block 512 kps 5 tiles_n 9 tiles_total 36 | none | ws 0 | wgrad K512 N2304 P147 x14x14x256 o7x7 f3x3 s2,2 p1,1
wgrad n3 14x14 c256 k512 1x1 s2,2 p0,0 e2 : igemm_wgrad_dma_kernel<128, 256, 2, 4> grid 4,1,1 block 512 kps 5 tiles_n 1 tiles_total 4 | none | ws 0 | wgrad K512 N256 P147 x14x14x256 o7x7 f1x1 s2,2 p0,0
wgrad n3 17x17 c128 k192 7x1 s1,1 p3,0 e2 : igemm_wgrad_dma_inc_kernel<128, 128, 2, 2> grid 14,1,1 block 256 kps 28 tiles_n 7 tiles_total 14 inc 15,1,17,17,4096,0,0 | none | ws 0 | wgrad K192 N896 P867 x17x17x128 o17x17 f7x1 s1,1 p3,0
wgrad n3 35x35 c48 k64 5x5 s1,1 p2,2 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 10,1,7 block 256 kps 17 tiles_n 10 tiles_total 10 inc 32,0,35,35,1536,0,0 | wgrad_reduce_kernel grid 300 | ws 537600 | wgrad K64 N1200 P3675 x35x35x48 o35x35 f5x5 s1,1 p2,2
wgrad n3 56x56 c256 k64 1x1 s1,1 p0,0 e2 : igemm_wgrad_dma_inc_kernel<64, 128, 2, 2> grid 2,1,18 block 256 kps 17 tiles_n 2 tiles_total 2 inc 32,0,56,56,8192,0,0 | wgrad_reduce_kernel grid 64 | ws 294912 | wgrad K64 N256 P9408 x56x56x256 o56x56 f1x1 s1,1 p0,0
"""  # noqa: E501

ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1",
           UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def check(request, tmp_path_factory):
    """Runs the check program, built once per variant, and returns its output."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("igemm_plan") / "igemm_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", "-I", KDIR, os.path.join(KDIR, "igemm_plan_check.cpp"), "-o", exe]
    if request.param != "plain":
        cmd.append("-fsanitize=" + request.param)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    return run


def test_every_swept_plan_is_inside_the_kernels_limits(check):
    assert "igemm_plan_check sweep ok" in check("sweep")


def test_model_zoo_dispatch(check):
    got, want = check().splitlines(), ZOO.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_shapes_and_switches_from_arguments(check):
    """A shape given as an argument plans like the built-in row; kpad=0 moves Inception's
    48-channel 5x5 from the padded uniform-tap kernel to the generic one (which may split
    again), dma_uni=0 leaves no uniform-tap or incremental kernel, a tuned or forced tile is
    honoured where its family has it, and engine=0 leaves no LDS-DMA family anywhere."""
    inception = "fwd:32,35,35,48,64,5,5,1,1,2,2,0"
    want = [ln for ln in ZOO.splitlines() if ln.startswith("fwd n32 35x35 c48 k64 5x5")]
    out = check("engine=1", inception, "kpad=0", inception).splitlines()
    assert out[0] == want[1]
    assert " : igemm_rows_dma_uni_kernel<128, 64, 2, 2, true, false, false> " in out[0]
    assert " Ktot 1600 kpad 1 " in out[0] and " | rows10 M39200 N64 K1600 " in out[0]
    assert " : igemm_rows_dma_kernel<128, 64, 2, 2, true, " in out[1]
    assert " Ktot 1200 kpad 0 " in out[1] and " | rows11 M39200 N64 K1200 " in out[1]

    layer = ["fwd:32,56,56,64,128,1,1,2,2,0,0,0", "wgrad:32,56,56,64,128,1,1,2,2,0,0",
             "dgrad:32,56,56,64,128,3,3,2,2,1,1,1"]
    out = check("engine=2", "dma_uni=0", *layer)
    assert "_dma_kernel<" in out and "_uni_kernel" not in out and "_inc_kernel" not in out
    out = check("engine=1", "tile=256,128", layer[0], "tile=0,0", "force=256,256,0", layer[0],
                "engine=0", layer[0]).splitlines()
    assert " : igemm_rows_dma_uni_kernel<256, 128, 2, 2, true, " in out[0]
    assert " : igemm_rows_dma_uni_kernel<256, 256, 2, 4, true, " in out[1] and " block 512 " in out[1]
    assert " : igemm_rows_kernel<128, 128, 2, 2, 8, true, " in out[2]  # (no 256x256 register tile)

    engine0 = [ln for ln in ZOO.splitlines() if " e0 : " in ln]
    assert len(engine0) > 100 and not any("_dma" in ln or ln.endswith("halo") for ln in engine0)
    assert engine0 == check("engine=0", *zoo_shapes(32), *zoo_shapes(3)).splitlines()


def zoo_shapes(batch):
    """The zoo's shapes as arguments, read from the check program's own list."""
    import re
    src = open(os.path.join(KDIR, "igemm_plan_check.cpp")).read()
    zoo = src[src.index("static const char* const ZOO[]"):]
    zoo = zoo[:zoo.index("};")]
    return [s % batch for s in re.findall(r'"([a-z]+:%d[0-9,]*)"', zoo)]

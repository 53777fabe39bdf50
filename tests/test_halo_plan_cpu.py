"""The halo 3x3 launch planner (``csrc/kernels/halo_plan.h``) on the host: the stand-alone
``csrc/kernels/halo_plan_check.cpp`` is built with the host compiler, plain and with
AddressSanitizer + UndefinedBehaviorSanitizer, and

* its sweep (image sizes x batches x channels x tap sets x epilogue flavours x switches x
  CU counts) finds every plan inside the limits the kernels state (grid, DMA counts, LDS,
  strip tiles, 32-bit offsets, 448-pixel tiles, ``halo_need``);
* the dispatch it prints for the model zoo's 3x3 / stride-1 layers is the table below -
  recorded from the launch code as it was before the planner existed (kernel symbol, grid,
  block and plan bytes of every launch), so a change of kernel, grid or tiling for one of
  these layers shows here, on the CPU;
* ``tools/halo_index_check.py``'s emulation of the geometry functions agrees with the header
  for every H, W in 1..64."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "csrc", "kernels")

# shape : kernel<template arguments> grid, block, tiles | plan fields.  conv3_halo_kernel<WRES,
# EPI, FULL, NJ, MI>, conv3_strip_kernel<WRES, EPI, NS, NJ>, conv3_halo_wgrad_kernel<W2T,
# ONECH, STRIP, PROD, KM, HT>; EPI 0 plain, 2 accumulate, 4 BN link, 8 statistics, 17 bias +
# ReLU.  (N == 96 is no column-tile width of the engine: Inception's 35 x 35 x 96 forward
# and dgrad run on the implicit GEMM.)
ZOO = """\
fwd b32 56x56 c64 n64 same stats ldc64 : conv3_halo_kernel<true, 8, true, 4, 7> grid 224 block 256 tiles_n 1 tiles_total 224 | w2 64 hiw 9 tiles_m 224 tiles_total 224 cc 2 a_bytes 12845056 b_bytes 73728
fwd b32 56x56 c64 n64 same_dgrad plain ldc64 : conv3_halo_kernel<true, 0, true, 4, 7> grid 224 block 256 tiles_n 1 tiles_total 224 | w2 64 hiw 9 tiles_m 224 tiles_total 224 cc 2 a_bytes 12845056 b_bytes 73728
fwd b32 56x56 c64 n64 same_dgrad acc ldc64 : conv3_halo_kernel<true, 2, true, 4, 4> grid 256 block 512 tiles_n 1 tiles_total 392 | w2 64 hiw 9 tiles_m 392 tiles_total 392 cc 2 a_bytes 12845056 b_bytes 73728
fwd b32 56x56 c64 n64 same_dgrad bnred ldc64 : conv3_halo_kernel<true, 4, true, 4, 4> grid 256 block 512 tiles_n 1 tiles_total 392 | w2 64 hiw 9 tiles_m 392 tiles_total 392 cc 2 a_bytes 12845056 b_bytes 73728
wgrad b32 56x56 c64 k64 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 256 block 512 | w2 64 tiles_m 784 parts 1 kparts 1 Z 256 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 12845056 x_bytes 12845056
fwd b3 56x56 c64 n64 same stats ldc64 : conv3_halo_kernel<true, 8, true, 4, 7> grid 24 block 256 tiles_n 1 tiles_total 21 | w2 64 hiw 9 tiles_m 21 tiles_total 21 cc 2 a_bytes 1204224 b_bytes 73728
fwd b3 56x56 c64 n64 same_dgrad plain ldc64 : conv3_halo_kernel<true, 0, true, 4, 7> grid 24 block 256 tiles_n 1 tiles_total 21 | w2 64 hiw 9 tiles_m 21 tiles_total 21 cc 2 a_bytes 1204224 b_bytes 73728
fwd b3 56x56 c64 n64 same_dgrad acc ldc64 : conv3_halo_kernel<true, 2, false, 4, 4> grid 40 block 512 tiles_n 1 tiles_total 37 | w2 64 hiw 9 tiles_m 37 tiles_total 37 cc 2 a_bytes 1204224 b_bytes 73728
fwd b3 56x56 c64 n64 same_dgrad bnred ldc64 : conv3_halo_kernel<true, 4, false, 4, 4> grid 40 block 512 tiles_n 1 tiles_total 37 | w2 64 hiw 9 tiles_m 37 tiles_total 37 cc 2 a_bytes 1204224 b_bytes 73728
wgrad b3 56x56 c64 k64 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 74 block 512 | w2 64 tiles_m 74 parts 1 kparts 1 Z 74 xmap 0 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 1204224 x_bytes 1204224
fwd b32 28x28 c128 n128 same stats ldc128 : conv3_halo_kernel<false, 8, true, 4, 4> grid 192 block 512 tiles_n 2 tiles_total 196 | w2 32 hiw 7 tiles_m 98 tiles_total 196 cc 4 a_bytes 6422528 b_bytes 294912
fwd b32 28x28 c128 n128 same_dgrad plain ldc128 : conv3_halo_kernel<false, 0, true, 4, 4> grid 192 block 512 tiles_n 2 tiles_total 196 | w2 32 hiw 7 tiles_m 98 tiles_total 196 cc 4 a_bytes 6422528 b_bytes 294912
fwd b32 28x28 c128 n128 same_dgrad acc ldc128 : conv3_halo_kernel<false, 2, true, 4, 4> grid 192 block 512 tiles_n 2 tiles_total 196 | w2 32 hiw 7 tiles_m 98 tiles_total 196 cc 4 a_bytes 6422528 b_bytes 294912
fwd b32 28x28 c128 n128 same_dgrad bnred ldc128 : conv3_halo_kernel<false, 4, true, 4, 4> grid 192 block 512 tiles_n 2 tiles_total 196 | w2 32 hiw 7 tiles_m 98 tiles_total 196 cc 4 a_bytes 6422528 b_bytes 294912
wgrad b32 28x28 c128 k128 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 256 block 512 | w2 32 tiles_m 196 parts 4 kparts 2 Z 64 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 6422528 x_bytes 6422528
fwd b3 28x28 c128 n128 same stats ldc128 : conv3_halo_kernel<false, 8, false, 4, 4> grid 16 block 512 tiles_n 2 tiles_total 20 | w2 32 hiw 7 tiles_m 10 tiles_total 20 cc 4 a_bytes 602112 b_bytes 294912
fwd b3 28x28 c128 n128 same_dgrad plain ldc128 : conv3_halo_kernel<false, 0, false, 4, 4> grid 16 block 512 tiles_n 2 tiles_total 20 | w2 32 hiw 7 tiles_m 10 tiles_total 20 cc 4 a_bytes 602112 b_bytes 294912
fwd b3 28x28 c128 n128 same_dgrad acc ldc128 : conv3_halo_kernel<false, 2, false, 4, 4> grid 16 block 512 tiles_n 2 tiles_total 20 | w2 32 hiw 7 tiles_m 10 tiles_total 20 cc 4 a_bytes 602112 b_bytes 294912
fwd b3 28x28 c128 n128 same_dgrad bnred ldc128 : conv3_halo_kernel<false, 4, false, 4, 4> grid 16 block 512 tiles_n 2 tiles_total 20 | w2 32 hiw 7 tiles_m 10 tiles_total 20 cc 4 a_bytes 602112 b_bytes 294912
wgrad b3 28x28 c128 k128 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 76 block 512 | w2 32 tiles_m 19 parts 4 kparts 2 Z 19 xmap 0 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 602112 x_bytes 602112
fwd b32 14x14 c256 n256 same stats ldc256 : conv3_halo_kernel<false, 8, false, 4, 4> grid 96 block 512 tiles_n 4 tiles_total 100 | w2 16 hiw 6 tiles_m 25 tiles_total 100 cc 8 a_bytes 3211264 b_bytes 1179648
fwd b32 14x14 c256 n256 same_dgrad plain ldc256 : conv3_halo_kernel<false, 0, false, 4, 4> grid 96 block 512 tiles_n 4 tiles_total 100 | w2 16 hiw 6 tiles_m 25 tiles_total 100 cc 8 a_bytes 3211264 b_bytes 1179648
fwd b32 14x14 c256 n256 same_dgrad acc ldc256 : conv3_halo_kernel<false, 2, false, 4, 4> grid 96 block 512 tiles_n 4 tiles_total 100 | w2 16 hiw 6 tiles_m 25 tiles_total 100 cc 8 a_bytes 3211264 b_bytes 1179648
fwd b32 14x14 c256 n256 same_dgrad bnred ldc256 : conv3_halo_kernel<false, 4, false, 4, 4> grid 96 block 512 tiles_n 4 tiles_total 100 | w2 16 hiw 6 tiles_m 25 tiles_total 100 cc 8 a_bytes 3211264 b_bytes 1179648
wgrad b32 14x14 c256 k256 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 256 block 512 | w2 16 tiles_m 49 parts 16 kparts 4 Z 16 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 3211264 x_bytes 3211264
fwd b3 14x14 c256 n256 same stats ldc256 : conv3_halo_kernel<false, 8, false, 4, 4> grid 32 block 512 tiles_n 4 tiles_total 12 | w2 16 hiw 6 tiles_m 3 tiles_total 12 cc 8 a_bytes 301056 b_bytes 1179648
fwd b3 14x14 c256 n256 same_dgrad plain ldc256 : conv3_halo_kernel<false, 0, false, 4, 4> grid 32 block 512 tiles_n 4 tiles_total 12 | w2 16 hiw 6 tiles_m 3 tiles_total 12 cc 8 a_bytes 301056 b_bytes 1179648
fwd b3 14x14 c256 n256 same_dgrad acc ldc256 : conv3_halo_kernel<false, 2, false, 4, 4> grid 32 block 512 tiles_n 4 tiles_total 12 | w2 16 hiw 6 tiles_m 3 tiles_total 12 cc 8 a_bytes 301056 b_bytes 1179648
fwd b3 14x14 c256 n256 same_dgrad bnred ldc256 : conv3_halo_kernel<false, 4, false, 4, 4> grid 32 block 512 tiles_n 4 tiles_total 12 | w2 16 hiw 6 tiles_m 3 tiles_total 12 cc 8 a_bytes 301056 b_bytes 1179648
wgrad b3 14x14 c256 k256 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 80 block 512 | w2 16 tiles_m 5 parts 16 kparts 4 Z 5 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 301056 x_bytes 301056
fwd b32 7x7 c512 n512 same stats ldc512 : conv3_halo_kernel<false, 8, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 56 | w2 8 hiw 6 tiles_m 7 tiles_total 56 cc 16 a_bytes 1605632 b_bytes 4718592
fwd b32 7x7 c512 n512 same_dgrad plain ldc512 : conv3_halo_kernel<false, 0, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 56 | w2 8 hiw 6 tiles_m 7 tiles_total 56 cc 16 a_bytes 1605632 b_bytes 4718592
fwd b32 7x7 c512 n512 same_dgrad acc ldc512 : conv3_halo_kernel<false, 2, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 56 | w2 8 hiw 6 tiles_m 7 tiles_total 56 cc 16 a_bytes 1605632 b_bytes 4718592
fwd b32 7x7 c512 n512 same_dgrad bnred ldc512 : conv3_halo_kernel<false, 4, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 56 | w2 8 hiw 6 tiles_m 7 tiles_total 56 cc 16 a_bytes 1605632 b_bytes 4718592
wgrad b32 7x7 c512 k512 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 256 block 512 | w2 16 tiles_m 13 parts 64 kparts 8 Z 4 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 1605632 x_bytes 1605632
fwd b3 7x7 c512 n512 same stats ldc512 : conv3_halo_kernel<false, 8, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 8 | w2 8 hiw 6 tiles_m 1 tiles_total 8 cc 16 a_bytes 150528 b_bytes 4718592
fwd b3 7x7 c512 n512 same_dgrad plain ldc512 : conv3_halo_kernel<false, 0, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 8 | w2 8 hiw 6 tiles_m 1 tiles_total 8 cc 16 a_bytes 150528 b_bytes 4718592
fwd b3 7x7 c512 n512 same_dgrad acc ldc512 : conv3_halo_kernel<false, 2, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 8 | w2 8 hiw 6 tiles_m 1 tiles_total 8 cc 16 a_bytes 150528 b_bytes 4718592
fwd b3 7x7 c512 n512 same_dgrad bnred ldc512 : conv3_halo_kernel<false, 4, false, 4, 4> grid 64 block 512 tiles_n 8 tiles_total 8 | w2 8 hiw 6 tiles_m 1 tiles_total 8 cc 16 a_bytes 150528 b_bytes 4718592
wgrad b3 7x7 c512 k512 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 128 block 512 | w2 16 tiles_m 2 parts 64 kparts 8 Z 2 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 150528 x_bytes 150528
fwd b32 224x224 c64 n64 same bias_relu ldc64 : conv3_strip_kernel<true, 17, 2, 4> grid 256 block 512 tiles_n 1 tiles_total 7168 | tr 2 tw 112 p 120 hiw 8 tiles_c 2 tiles_img 224 tiles_total 7168 cc 2 ch 0 cw 0 a_bytes 205520896 b_bytes 73728
wgrad b32 224x224 c64 k64 pad1 : conv3_halo_wgrad_kernel<0, false, true, false, 4, 7> grid 256 block 256 | w2 16 tiles_m 12800 parts 1 kparts 1 Z 256 xmap 1 tr 9 tw 14 tiles_c 16 tiles_img 400 dy_bytes 205520896 x_bytes 205520896
fwd b32 112x112 c128 n128 same bias_relu ldc128 : conv3_strip_kernel<false, 17, 2, 4> grid 256 block 512 tiles_n 2 tiles_total 3584 | tr 2 tw 112 p 120 hiw 8 tiles_c 1 tiles_img 56 tiles_total 3584 cc 4 ch 0 cw 0 a_bytes 102760448 b_bytes 294912
wgrad b32 112x112 c128 k128 pad1 : conv3_halo_wgrad_kernel<0, false, true, false, 4, 7> grid 256 block 256 | w2 16 tiles_m 3328 parts 4 kparts 2 Z 64 xmap 1 tr 9 tw 14 tiles_c 8 tiles_img 104 dy_bytes 102760448 x_bytes 102760448
fwd b32 56x56 c128 n32 same plain ldc96 : conv3_halo_kernel<false, 0, true, 2, 4> grid 256 block 512 tiles_n 1 tiles_total 392 | w2 64 hiw 9 tiles_m 392 tiles_total 392 cc 4 a_bytes 25690112 b_bytes 73728
wgrad b32 56x56 c128 k32 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 2, 7> grid 256 block 512 | w2 64 tiles_m 784 parts 2 kparts 1 Z 128 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 6422528 x_bytes 25690112
fwd b32 7x7 c128 n32 same plain ldc96 : conv3_halo_kernel<false, 0, false, 2, 4> grid 8 block 512 tiles_n 1 tiles_total 7 | w2 8 hiw 6 tiles_m 7 tiles_total 7 cc 4 a_bytes 401408 b_bytes 73728
wgrad b32 7x7 c128 k32 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 2, 7> grid 26 block 512 | w2 16 tiles_m 13 parts 2 kparts 1 Z 13 xmap 0 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 100352 x_bytes 401408
fwd b32 149x149 c32 n32 valid stats ldc32 : conv3_strip_kernel<true, 8, 3, 2> grid 256 block 512 tiles_n 1 tiles_total 3136 | tr 3 tw 74 p 80 hiw 7 tiles_c 2 tiles_img 98 tiles_total 3136 cc 1 ch 1 cw 1 a_bytes 45467648 b_bytes 18432
fwd b32 149x149 c32 n32 valid_dgrad plain ldc32 : conv3_strip_kernel<true, 0, 3, 2> grid 256 block 512 tiles_n 1 tiles_total 3200 | tr 3 tw 75 p 80 hiw 7 tiles_c 2 tiles_img 100 tiles_total 3200 cc 1 ch -1 cw -1 a_bytes 44255232 b_bytes 18432
wgrad b32 149x149 c32 k32 pad0 : conv3_halo_wgrad_kernel<0, false, true, false, 4, 7> grid 256 block 256 | w2 16 tiles_m 5984 parts 1 kparts 1 Z 256 xmap 1 tr 9 tw 14 tiles_c 11 tiles_img 187 dy_bytes 44255232 x_bytes 45467648
fwd b32 147x147 c32 n64 same stats ldc64 : conv3_strip_kernel<true, 8, 3, 4> grid 256 block 512 tiles_n 1 tiles_total 3136 | tr 3 tw 74 p 80 hiw 7 tiles_c 2 tiles_img 98 tiles_total 3136 cc 1 ch 0 cw 0 a_bytes 44255232 b_bytes 36864
fwd b32 147x147 c64 n32 same_dgrad plain ldc32 : conv3_strip_kernel<true, 0, 2, 2> grid 256 block 512 tiles_n 1 tiles_total 3136 | tr 3 tw 74 p 80 hiw 7 tiles_c 2 tiles_img 98 tiles_total 3136 cc 2 ch 0 cw 0 a_bytes 88510464 b_bytes 36864
wgrad b32 147x147 c32 k64 pad1 : conv3_halo_wgrad_kernel<0, true, false, true, 4, 7> grid 256 block 512 | w2 160 tiles_m 5403 parts 1 kparts 1 Z 256 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 88510464 x_bytes 44255232
fwd b32 35x35 c96 n96 same stats ldc96 : none
fwd b32 35x35 c96 n96 same_dgrad plain ldc96 : none
wgrad b32 35x35 c96 k96 pad1 : conv3_halo_wgrad_kernel<0, false, false, true, 4, 7> grid 256 block 512 | w2 48 tiles_m 307 parts 4 kparts 2 Z 64 xmap 1 tr 0 tw 0 tiles_c 0 tiles_img 0 dy_bytes 7526400 x_bytes 7526400
"""  # noqa: E501

ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1",
           UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def check(request, tmp_path_factory):
    """Runs the check program, built once per variant, and returns its output."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("halo_plan") / "halo_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", "-I", KDIR, os.path.join(KDIR, "halo_plan_check.cpp"), "-o", exe]
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
    assert "halo_plan_check sweep ok" in check("sweep")


def test_model_zoo_dispatch(check):
    got, want = check().splitlines(), ZOO.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_shapes_and_switches_from_arguments(check):
    """A shape given as an argument plans like the built-in row; MPA_HALO_STRIP=2 moves
    ResNet layer1 to three-stage strips, MPA_HALO=0 off the engine."""
    row = "fwd:32,56,56,64,64,same,stats,0"
    out = check(row, "strip=2", row, "halo=0", row, "wgrad:32,56,56,64,64,1").splitlines()
    assert out[0] == ZOO.splitlines()[0]
    assert " : conv3_strip_kernel<true, 8, 3, 4> grid 256 block 512 " in out[1]
    assert out[2].endswith(" : none") and out[3].endswith(" : none")


def test_index_tool_emulates_the_header(check):
    """tools/halo_index_check.py's halo_need / dma_count / pitches are the header's."""
    spec = importlib.util.spec_from_file_location(
        "halo_index_check", os.path.join(ROOT, "tools", "halo_index_check.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = {}
    for ln in check("geometry").splitlines():
        v = [int(x) for x in ln.split()]
        rows[v[0], v[1]] = v[2:]
    assert sorted(rows) == [(h, w) for h in range(1, 65) for w in range(1, 65)]
    for (h, w), (pf, nf, cf, pw, nw, cw, _inst) in rows.items():
        assert (tool.fwd_pitch(w), tool.wgrad_pitch(w)) == (pf, pw), (h, w)
        assert tool.halo_need(256, h, w, pf) == nf and tool.halo_need(128, h, w, pw) == nw, (h, w)
        assert tool.dma_count(nf, 9) == cf and tool.dma_count(nw, 7) == cw, (h, w)
    for w, (f, g) in tool.TABLE.items():  # the ResNet layers' counts
        assert tuple(rows[w, w][i] for i in (2, 5)) == (f, g), w
        assert rows[w, w][6] == g, w  # (each of these counts is instantiated for its pitch)

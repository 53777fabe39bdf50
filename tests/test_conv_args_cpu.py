"""From a layer's shape to its GEMM launch arguments (``csrc/kernels/conv_args.h``) on the
host: the stand-alone ``csrc/kernels/conv_args_check.cpp`` is built with the host compiler,
plain and with AddressSanitizer + UndefinedBehaviorSanitizer, and

* its sweep interprets the arguments of every shape - forward (plain and 8-channel
  super-tap), dgrad for strides 1..3 from either weight layout, dgrad pairs, one-tap
  launches - on integer data and finds exactly the textbook convolution / transposed
  convolution, every dx pixel stored by exactly one stride phase (or by none where the
  phase has no taps), and no tap index at the table's end;
* the weight-gradient fields of the same shapes equal their definitions;
* the arguments it prints for layers of the model zoo are the lines below - recorded from
  the binding layer's own loops as they were before the header existed, so a change of any
  field, tap or phase for one of these layers shows here, on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "csrc", "kernels")

# shape : a (gathered tensor) o (rows' grid) M U / O (gather stride / origin) T Ktot N RS ldb
# d (output grid) Uo / Po (output stride / origin) ... | taps dh,dw,bt | stride phases |
# whether a phase had no taps.  A strided dgrad has no single-launch fields (o 0x0 M 0 T 0).
ZOO = """\
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap1 : a 224x224x8 o 112x112 M 401408 U 2,2 O -3,-3 T 14 Ktot 448 N 64 RS 49 ldb 392 d 112x112 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 1 ldb2 0 | taps 0,0,0x4000 0,4,0x3004 1,0,0x4007 1,4,0x300b 2,0,0x400e 2,4,0x3012 3,0,0x4015 3,4,0x3019 4,0,0x401c 4,4,0x3020 5,0,0x4023 5,4,0x3027 6,0,0x402a 6,4,0x302e | ph | empty 0
fwd n32 224x224 c8 k64 7x7 s2,2 p3,3 stap0 : a 224x224x8 o 112x112 M 401408 U 2,2 O -3,-3 T 49 Ktot 392 N 64 RS 49 ldb 392 d 112x112 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 0,1,0x1 0,2,0x2 0,3,0x3 0,4,0x4 0,5,0x5 0,6,0x6 1,0,0x7 1,1,0x8 1,2,0x9 1,3,0xa 1,4,0xb 1,5,0xc 1,6,0xd 2,0,0xe 2,1,0xf 2,2,0x10 2,3,0x11 2,4,0x12 2,5,0x13 2,6,0x14 3,0,0x15 3,1,0x16 3,2,0x17 3,3,0x18 3,4,0x19 3,5,0x1a 3,6,0x1b 4,0,0x1c 4,1,0x1d 4,2,0x1e 4,3,0x1f 4,4,0x20 4,5,0x21 4,6,0x22 5,0,0x23 5,1,0x24 5,2,0x25 5,3,0x26 5,4,0x27 5,5,0x28 5,6,0x29 6,0,0x2a 6,1,0x2b 6,2,0x2c 6,3,0x2d 6,4,0x2e 6,5,0x2f 6,6,0x30 | ph | empty 0
dgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 wt0 : a 112x112x64 o 0x0 M 0 U 1,1 O 0,0 T 0 Ktot 0 N 8 RS 49 ldb 8 d 224x224 Uo 2,2 Po 0,0 nphase 4 tapmap 0 stap 0 ldb2 0 | taps 1,1,0x8 1,0,0xa 1,-1,0xc 0,1,0x16 0,0,0x18 0,-1,0x1a -1,1,0x24 -1,0,0x26 -1,-1,0x28 1,2,0x7 1,1,0x9 1,0,0xb 1,-1,0xd 0,2,0x15 0,1,0x17 0,0,0x19 0,-1,0x1b -1,2,0x23 -1,1,0x25 -1,0,0x27 -1,-1,0x29 2,1,0x1 2,0,0x3 2,-1,0x5 1,1,0xf 1,0,0x11 1,-1,0x13 0,1,0x1d 0,0,0x1f 0,-1,0x21 -1,1,0x2b -1,0,0x2d -1,-1,0x2f 2,2,0 2,1,0x2 2,0,0x4 2,-1,0x6 1,2,0xe 1,1,0x10 1,0,0x12 1,-1,0x14 0,2,0x1c 0,1,0x1e 0,0,0x20 0,-1,0x22 -1,2,0x2a -1,1,0x2c -1,0,0x2e -1,-1,0x30 | ph [M 401408 o 112x112 Ktot 576 taps 0+9 Po 0,0] [M 401408 o 112x112 Ktot 768 taps 9+12 Po 0,1] [M 401408 o 112x112 Ktot 768 taps 21+12 Po 1,0] [M 401408 o 112x112 Ktot 1024 taps 33+16 Po 1,1] | empty 0
wgrad n32 224x224 c8 k64 7x7 s2,2 p3,3 : Kout 64 C 8 x 224x224 dy 112x112 w 7x7 s 2,2 p 3,3 Mpix 401408 Ncols 392 overwrite 0
fwd n32 56x56 c64 k64 3x3 s1,1 p1,1 stap0 : a 56x56x64 o 56x56 M 100352 U 1,1 O -1,-1 T 9 Ktot 576 N 64 RS 9 ldb 576 d 56x56 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 0,1,0x1 0,2,0x2 1,0,0x3 1,1,0x4 1,2,0x5 2,0,0x6 2,1,0x7 2,2,0x8 | ph | empty 0
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt1 : a 56x56x64 o 56x56 M 100352 U 1,1 O 0,0 T 9 Ktot 576 N 64 RS 9 ldb 576 d 56x56 Uo 1,1 Po 0,0 nphase 0 tapmap 1 stap 0 ldb2 0 | taps 1,1,0 1,0,0x1 1,-1,0x2 0,1,0x3 0,0,0x4 0,-1,0x5 -1,1,0x6 -1,0,0x7 -1,-1,0x8 | ph | empty 0
dgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 wt0 : a 56x56x64 o 56x56 M 100352 U 1,1 O 0,0 T 9 Ktot 576 N 64 RS 9 ldb 64 d 56x56 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 1,1,0 1,0,0x1 1,-1,0x2 0,1,0x3 0,0,0x4 0,-1,0x5 -1,1,0x6 -1,0,0x7 -1,-1,0x8 | ph | empty 0
wgrad n32 56x56 c64 k64 3x3 s1,1 p1,1 : Kout 64 C 64 x 56x56 dy 56x56 w 3x3 s 1,1 p 1,1 Mpix 100352 Ncols 576 overwrite 0
fwd n32 56x56 c64 k128 3x3 s2,2 p1,1 stap0 : a 56x56x64 o 28x28 M 25088 U 2,2 O -1,-1 T 9 Ktot 576 N 128 RS 9 ldb 576 d 28x28 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 0,1,0x1 0,2,0x2 1,0,0x3 1,1,0x4 1,2,0x5 2,0,0x6 2,1,0x7 2,2,0x8 | ph | empty 0
dgrad n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 : a 28x28x128 o 0x0 M 0 U 1,1 O 0,0 T 0 Ktot 0 N 64 RS 9 ldb 1152 d 56x56 Uo 2,2 Po 0,0 nphase 4 tapmap 1 stap 0 ldb2 0 | taps 0,0,0x4 0,1,0x3 0,0,0x5 1,0,0x1 0,0,0x7 1,1,0 1,0,0x2 0,1,0x6 0,0,0x8 | ph [M 25088 o 28x28 Ktot 128 taps 0+1 Po 0,0] [M 25088 o 28x28 Ktot 256 taps 1+2 Po 0,1] [M 25088 o 28x28 Ktot 256 taps 3+2 Po 1,0] [M 25088 o 28x28 Ktot 512 taps 5+4 Po 1,1] | empty 0
pair n32 56x56 c64 k128 3x3 s2,2 p1,1 wt1 + 1x1 p0,0 : a 28x28x128 o 0x0 M 0 U 1,1 O 0,0 T 0 Ktot 0 N 64 RS 9 ldb 1152 d 56x56 Uo 2,2 Po 0,0 nphase 4 tapmap 1 stap 0 ldb2 128 | taps 0,0,0x4 0,0,0x2000 0,1,0x3 0,0,0x5 1,0,0x1 0,0,0x7 1,1,0 1,0,0x2 0,1,0x6 0,0,0x8 | ph [M 25088 o 28x28 Ktot 256 taps 0+2 Po 0,0] [M 25088 o 28x28 Ktot 256 taps 2+2 Po 0,1] [M 25088 o 28x28 Ktot 256 taps 4+2 Po 1,0] [M 25088 o 28x28 Ktot 512 taps 6+4 Po 1,1] | empty 0
fwd n32 56x56 c64 k128 1x1 s2,2 p0,0 stap0 : a 56x56x64 o 28x28 M 25088 U 2,2 O 0,0 T 1 Ktot 64 N 128 RS 1 ldb 64 d 28x28 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 | ph | empty 0
dgrad n32 56x56 c64 k128 1x1 s2,2 p0,0 wt1 : a 28x28x128 o 0x0 M 0 U 1,1 O 0,0 T 0 Ktot 0 N 64 RS 1 ldb 128 d 56x56 Uo 2,2 Po 0,0 nphase 1 tapmap 1 stap 0 ldb2 0 | taps 0,0,0 | ph [M 25088 o 28x28 Ktot 128 taps 0+1 Po 0,0] | empty 1
fwd n32 17x17 c128 k128 1x7 s1,1 p0,3 stap0 : a 17x17x128 o 17x17 M 9248 U 1,1 O 0,-3 T 7 Ktot 896 N 128 RS 7 ldb 896 d 17x17 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 0,1,0x1 0,2,0x2 0,3,0x3 0,4,0x4 0,5,0x5 0,6,0x6 | ph | empty 0
dgrad n32 17x17 c128 k128 1x7 s1,1 p0,3 wt1 : a 17x17x128 o 17x17 M 9248 U 1,1 O 0,0 T 7 Ktot 896 N 128 RS 7 ldb 896 d 17x17 Uo 1,1 Po 0,0 nphase 0 tapmap 1 stap 0 ldb2 0 | taps 0,3,0 0,2,0x1 0,1,0x2 0,0,0x3 0,-1,0x4 0,-2,0x5 0,-3,0x6 | ph | empty 0
fwd n32 17x17 c128 k192 7x1 s1,1 p3,0 stap0 : a 17x17x128 o 17x17 M 9248 U 1,1 O -3,0 T 7 Ktot 896 N 192 RS 7 ldb 896 d 17x17 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 1,0,0x1 2,0,0x2 3,0,0x3 4,0,0x4 5,0,0x5 6,0,0x6 | ph | empty 0
dgrad n32 17x17 c128 k192 7x1 s1,1 p3,0 wt1 : a 17x17x192 o 17x17 M 9248 U 1,1 O 0,0 T 7 Ktot 1344 N 128 RS 7 ldb 1344 d 17x17 Uo 1,1 Po 0,0 nphase 0 tapmap 1 stap 0 ldb2 0 | taps 3,0,0 2,0,0x1 1,0,0x2 0,0,0x3 -1,0,0x4 -2,0,0x5 -3,0,0x6 | ph | empty 0
fwd n32 35x35 c288 k384 3x3 s2,2 p0,0 stap0 : a 35x35x288 o 17x17 M 9248 U 2,2 O 0,0 T 9 Ktot 2592 N 384 RS 9 ldb 2592 d 17x17 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 0,1,0x1 0,2,0x2 1,0,0x3 1,1,0x4 1,2,0x5 2,0,0x6 2,1,0x7 2,2,0x8 | ph | empty 0
dgrad n32 35x35 c288 k384 3x3 s2,2 p0,0 wt1 : a 17x17x384 o 0x0 M 0 U 1,1 O 0,0 T 0 Ktot 0 N 288 RS 9 ldb 3456 d 35x35 Uo 2,2 Po 0,0 nphase 4 tapmap 1 stap 0 ldb2 0 | taps 0,0,0 0,-1,0x2 -1,0,0x6 -1,-1,0x8 0,0,0x1 -1,0,0x7 0,0,0x3 0,-1,0x5 0,0,0x4 | ph [M 10368 o 18x18 Ktot 1536 taps 0+4 Po 0,0] [M 9792 o 18x17 Ktot 768 taps 4+2 Po 0,1] [M 9792 o 17x18 Ktot 768 taps 6+2 Po 1,0] [M 9248 o 17x17 Ktot 384 taps 8+1 Po 1,1] | empty 0
fwd n32 35x35 c48 k64 5x5 s1,1 p2,2 stap0 : a 35x35x48 o 35x35 M 39200 U 1,1 O -2,-2 T 25 Ktot 1200 N 64 RS 25 ldb 1200 d 35x35 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 0,1,0x1 0,2,0x2 0,3,0x3 0,4,0x4 1,0,0x5 1,1,0x6 1,2,0x7 1,3,0x8 1,4,0x9 2,0,0xa 2,1,0xb 2,2,0xc 2,3,0xd 2,4,0xe 3,0,0xf 3,1,0x10 3,2,0x11 3,3,0x12 3,4,0x13 4,0,0x14 4,1,0x15 4,2,0x16 4,3,0x17 4,4,0x18 | ph | empty 0
dgrad n32 35x35 c48 k64 5x5 s1,1 p2,2 wt1 : a 35x35x64 o 35x35 M 39200 U 1,1 O 0,0 T 25 Ktot 1600 N 48 RS 25 ldb 1600 d 35x35 Uo 1,1 Po 0,0 nphase 0 tapmap 1 stap 0 ldb2 0 | taps 2,2,0 2,1,0x1 2,0,0x2 2,-1,0x3 2,-2,0x4 1,2,0x5 1,1,0x6 1,0,0x7 1,-1,0x8 1,-2,0x9 0,2,0xa 0,1,0xb 0,0,0xc 0,-1,0xd 0,-2,0xe -1,2,0xf -1,1,0x10 -1,0,0x11 -1,-1,0x12 -1,-2,0x13 -2,2,0x14 -2,1,0x15 -2,0,0x16 -2,-1,0x17 -2,-2,0x18 | ph | empty 0
fwd n32 56x56 c128 k128 1x1 s1,1 p0,0 stap0 : a 56x56x128 o 56x56 M 100352 U 1,1 O 0,0 T 1 Ktot 128 N 128 RS 1 ldb 128 d 56x56 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 | ph | empty 0
pointwise n32 56x56 c128 k64 ldb128 tapmap1 : a 56x56x128 o 56x56 M 100352 U 1,1 O 0,0 T 1 Ktot 128 N 64 RS 1 ldb 128 d 56x56 Uo 1,1 Po 0,0 nphase 0 tapmap 1 stap 0 ldb2 0 | taps 0,0,0 | ph | empty 0
pointwise n32 1x1 c512 k1000 ldb512 tapmap0 : a 1x1x512 o 1x1 M 32 U 1,1 O 0,0 T 1 Ktot 512 N 1000 RS 1 ldb 512 d 1x1 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 | ph | empty 0
pointwise n32 1x1 c1000 k512 ldb512 tapmap0 : a 1x1x1000 o 1x1 M 32 U 1,1 O 0,0 T 1 Ktot 1000 N 512 RS 1 ldb 512 d 1x1 Uo 1,1 Po 0,0 nphase 0 tapmap 0 stap 0 ldb2 0 | taps 0,0,0 | ph | empty 0
wgrad n32 1x1 c512 k1000 1x1 s1,1 p0,0 : Kout 1000 C 512 x 1x1 dy 1x1 w 1x1 s 1,1 p 0,0 Mpix 32 Ncols 512 overwrite 0
"""  # noqa: E501

# the shapes of ZOO, in its order: the ResNet stem (super-tap and plain form, its dgrad and
# weight gradient), a 3x3/s1, a 3x3/s2 alone and with its 1x1/s2 shortcut, the 1x1/s2 (three
# of its four phases have no taps), Inception's 1x7 / 7x1 / 3x3/s2 valid / 5x5/p2,
# DenseNet's 1x1 and its one-tap fused dgrad, a linear layer's forward, dgrad and wgrad
SHAPES = """\
fwd:32,224,224,8,64,7,7,2,2,3,3,1 fwd:32,224,224,8,64,7,7,2,2,3,3,0
dgrad:32,224,224,8,64,7,7,2,2,3,3,0 wgrad:32,224,224,8,64,7,7,2,2,3,3
fwd:32,56,56,64,64,3,3,1,1,1,1,0 dgrad:32,56,56,64,64,3,3,1,1,1,1,1
dgrad:32,56,56,64,64,3,3,1,1,1,1,0 wgrad:32,56,56,64,64,3,3,1,1,1,1
fwd:32,56,56,64,128,3,3,2,2,1,1,0 dgrad:32,56,56,64,128,3,3,2,2,1,1,1
pair:32,56,56,64,128,3,3,2,2,1,1,1,1,0,0
fwd:32,56,56,64,128,1,1,2,2,0,0,0 dgrad:32,56,56,64,128,1,1,2,2,0,0,1
fwd:32,17,17,128,128,1,7,1,1,0,3,0 dgrad:32,17,17,128,128,1,7,1,1,0,3,1
fwd:32,17,17,128,192,7,1,1,1,3,0,0 dgrad:32,17,17,128,192,7,1,1,1,3,0,1
fwd:32,35,35,288,384,3,3,2,2,0,0,0 dgrad:32,35,35,288,384,3,3,2,2,0,0,1
fwd:32,35,35,48,64,5,5,1,1,2,2,0 dgrad:32,35,35,48,64,5,5,1,1,2,2,1
fwd:32,56,56,128,128,1,1,1,1,0,0,0 pointwise:32,56,56,128,64,128,1
pointwise:32,1,1,512,1000,512,0 pointwise:32,1,1,1000,512,512,0
wgrad:32,1,1,512,1000,1,1,1,1,0,0
""".split()

ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 detect_leaks=1",
           UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def check(request, tmp_path_factory):
    """Runs the check program, built once per variant, and returns its output."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("conv_args") / "conv_args_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Werror", "-I", KDIR, os.path.join(KDIR, "conv_args_check.cpp"), "-o", exe]
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


def test_every_swept_shape_executes_to_the_textbook_result(check):
    """249,553 launches interpreted and equal to the reference, element for element."""
    assert check("sweep") == (
        "conv_args_check sweep ok: 249553 shapes executed (85962 fwd, 123488 dgrad, 39995 pair, "
        "108 pointwise), 11156 skipped (empty output)\n")


def test_wgrad_fields_equal_their_definitions(check):
    assert check("wgrad") == "conv_args_check wgrad ok: 74096 shapes\n"


def test_model_zoo_arguments(check):
    got, want = check("dump", *SHAPES).splitlines(), ZOO.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want) == len(SHAPES)


def test_one_shape_from_arguments(check):
    """`exec` interprets the shapes given: a small stem, a 3x3/s2 with its 1x1/s2 shortcut,
    and a 1x1/s2 whose tap-less phases leave dx pixels to the zero fill."""
    out = check("exec", "fwd:2,9,9,8,3,7,7,2,2,3,3,1", "pair:2,9,9,3,2,3,3,2,2,1,1,1,1,0,0",
                "dgrad:1,5,5,2,2,1,1,2,2,0,0,1").splitlines()
    assert len(out) == 3 and all(ln.endswith(" : exec ok") for ln in out)

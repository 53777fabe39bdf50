"""Host emulation of conv_halo.hip's index math (no GPU): for every 256-pixel tile, fill the
LDS halo image exactly as the DMA lanes do (slot / column / separator mapping with the
magic-number divisions, slot blocks dealt round-robin over the four DMA waves and bounded
by the geometry-sized per-wave DMA count) and check that every fragment read of every tap
lands on the right input pixel (or on a zero), in a slot that was fetched and that lies
below `need`, the slot count the host sizes the fetch by.  Run before launching a changed
kernel:  python tools/halo_index_check.py

The definition of halo_need, the DMA count and the two pitches is csrc/kernels/halo_plan.h
(what the host launches); the functions of those names here are an emulation of it, checked
against the header for every H, W in 1..64 by tests/test_halo_plan_cpu.py."""
import itertools

NW = 4  # DMA waves per block; one DMA instruction fetches a block of 16 slots


def magic(d):
    return (1 << 32) // d + 1


def udiv(n, m):
    return (n * m) >> 32


def halo_need(BM, H, W, W2):
    """halo_plan.h halo_need(): slots any BM-pixel linear tile can read - the rows it
    touches, 2 halo rows and the image separators it crosses, times the pitch (+1: with
    pitch W + 1 the last slot's right border is the next pixel)."""
    rows = (BM - 1 + W - 1) // W + 1
    seps = (BM - 1) // (H * W) + 1
    return (rows + 2 + seps) * W2 + (1 if W2 == W + 1 else 0)


def dma_count(need, hiw_max):
    """halo_plan.h halo_dma_count(): 16-slot DMA instructions per wave covering `need`"""
    blocks = (need + 15) // 16
    return min(hiw_max, (blocks + NW - 1) // NW)


def check(N, H, W, BM=256, HPX=576, pitch=None, trim=True):
    HW, W2 = H * W, (pitch(W) if pitch else W + 2)
    M = N * HW
    need = halo_need(BM, H, W, W2)
    if need > HPX:
        return "not eligible"
    hiw = dma_count(need, HPX // (16 * NW)) if trim else HPX // (16 * NW)
    mw2, mh1, mhw, mw = magic(W2), magic(H + 1), magic(HW), magic(W)
    for mt in range((M + BM - 1) // BM):
        m0 = mt * BM
        img0 = m0 // HW
        oh0 = (m0 - img0 * HW) // W
        lds = {}
        # DMA instruction j of wave w fetches slot block q = j * NW + w (LDS byte q * 1024)
        for j, wave, lane4 in itertools.product(range(hiw), range(NW), range(16)):
            hp = 16 * (j * NW + wave) + lane4
            s = udiv(hp, mw2)
            col = hp - s * W2 - 1
            v = s + oh0 - 1
            d = udiv(v + H + 1, mh1) - 1
            row = v - d * (H + 1)
            img = img0 + d
            assert hp not in lds and hp < HPX
            lds[hp] = (img, row, col) if (row < H and 0 <= col < W and img < N) else None
        assert sorted(lds) == list(range(64 * hiw))
        r0 = m0 - img0 * HW
        mlast = M - 1 - img0 * HW
        for rel in range(BM):  # (rows past M read the last pixel's slots: included)
            n = min(r0 + rel, mlast)
            di = udiv(n, mhw)
            rem = n - di * HW
            oh = udiv(rem, mw)
            ow = rem - oh * W
            assert di == n // HW and oh == rem // W
            hpb = ((di * (H + 1) + oh) - oh0 + 1) * W2 + ow + 1
            for dh, dw in itertools.product((-1, 0, 1), repeat=2):
                hp = hpb + dh * W2 + dw
                assert 0 <= hp < need, (N, H, W, mt, rel, hp, need)
                assert hp in lds, (N, H, W, mt, rel, hp, "never fetched")
                r, c = oh + dh, ow + dw
                exp = (img0 + di, r, c) if (0 <= r < H and 0 <= c < W) else None
                assert lds[hp] == exp, (N, H, W, mt, rel, dh, dw, lds[hp], exp)
    return "ok, %d of %d DMAs" % (hiw, HPX // (16 * NW))


def fwd_pitch(w):
    return (w + 1 + 7) // 8 * 8


def wgrad_pitch(w):
    return (w + 2 + 15) // 16 * 16


CASES = [(2, 56, 56), (3, 28, 28), (5, 14, 14), (7, 7, 7), (3, 9, 11), (1, 5, 3),
         (2, 35, 35), (4, 1, 1), (3, 2, 2), (64, 7, 7), (2, 17, 17)]
# the ResNet image widths with 1, 2 and 3 images (tail tiles, separators, clamped rows)
CASES += [(n, w, w) for w in (56, 28, 14, 7) for n in (1, 2, 3)]

# per-wave DMA counts of the ResNet layers: width -> (forward / dgrad of 9, wgrad of 7)
TABLE = {56: (9, 7), 28: (7, 5), 14: (6, 4), 7: (6, 7)}


def run(out=print):
    for w, (f, g) in TABLE.items():
        assert dma_count(halo_need(256, w, w, fwd_pitch(w)), 9) == f, w
        assert dma_count(halo_need(128, w, w, wgrad_pitch(w)), 7) == g, w
    for case in CASES:
        for trim in (True, False):
            out(case, "trim" if trim else "full",
                "fwd/dgrad (256-px tiles, pitch W+1 -> x8):",
                check(*case, pitch=fwd_pitch, trim=trim),
                "| wgrad (128-px tiles, pitch W+2 -> x16):",
                check(*case, BM=128, HPX=448, pitch=wgrad_pitch, trim=trim))


if __name__ == "__main__":
    run()

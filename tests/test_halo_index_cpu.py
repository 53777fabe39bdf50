"""tools/halo_index_check.py on the host: the emulated DMA fill of the 3x3 halo kernels
(round-robin slot blocks, geometry-sized DMA count) serves every fragment read of every tap
of every tile - tail tiles and clamped rows included - from a fetched slot below `need`."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "halo_index_check", os.path.join(ROOT, "tools", "halo_index_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_halo_reads_stay_below_need():
    tool = _tool()
    lines = []
    tool.run(out=lambda *a: lines.append(" ".join(str(x) for x in a)))
    # every ResNet width with 1, 2 and 3 images was checked in both tilings
    for w in (56, 28, 14, 7):
        for n in (1, 2, 3):
            row = [ln for ln in lines if ln.startswith("(%d, %d, %d) trim" % (n, w, w))]
            assert row and row[0].count("ok,") == 2, (n, w, row)


def test_halo_check_sees_a_short_fetch():
    """One DMA instruction per wave fewer than the geometry needs is caught."""
    tool = _tool()
    real = tool.dma_count
    tool.dma_count = lambda need, hiw_max: real(need, hiw_max) - 1
    try:
        for kw in (dict(pitch=tool.fwd_pitch), dict(BM=128, HPX=448, pitch=tool.wgrad_pitch)):
            try:
                tool.check(3, 28, 28, **kw)
            except AssertionError:
                continue
            raise RuntimeError("a short fetch went unnoticed: %r" % (kw,))
    finally:
        tool.dma_count = real

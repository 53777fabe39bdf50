"""bench.py's workload with the weight EMA on: the same flags, the same JSON result line,
``build_training`` called with ``ema_decay`` (default 0.9998, with the warm-up).  For A/B
pairs against plain ``bench.py`` - the benchmark itself stays as it is.  One process only
(``--gpus 1``): more ranks would re-launch ``bench.py``, without the EMA.

    python tools/ema_bench.py [--ema-decay 0.9998] --gpus 1 --steps 60 --warmup 10
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    decay = 0.9998
    if "--ema-decay" in argv:
        i = argv.index("--ema-decay")
        decay = float(argv[i + 1])
        del argv[i:i + 2]
    import bench
    import mpi_pytorch_amd.engine as engine
    if bench.parse_args(argv).gpus != 1:
        raise SystemExit("tools/ema_bench.py: --gpus 1 only")
    real = engine.build_training

    def build_training(*a, **kw):
        kw.setdefault("ema_decay", decay)
        out = real(*a, **kw)
        assert out[2].ema is not None
        print("ema_bench: weight EMA on, decay {}".format(out[2].ema.decay), file=sys.stderr)
        return out

    engine.build_training = build_training  # (bench.run imports it from the package)
    try:
        bench.main(argv)
    finally:
        engine.build_training = real


if __name__ == "__main__":
    main()

"""Kernel-call trace of one training step (forward, backward, optimizer) per model: every
call through the namespace ``Fn.K`` returns, as ``name(tensor-argument shapes)``, in order.
Two trees launch the same kernels iff their traces are equal - compare the printed
sha256 (or the ``--out`` files); ``grad`` is the sha256 of the gradient arena's bytes.

    python tools/op_trace.py [--device cpu|cuda] [--batch B] [--out DIR] model@size ...
Not part of the test suite."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mpi_pytorch_amd.engine import build_training
from mpi_pytorch_amd.ops import functional as Fn
from mpi_pytorch_amd.parallel import World


class Traced:
    """A kernel namespace that appends every call it passes through to ``log``."""

    def __init__(self, mod, log):
        self._mod, self._log = mod, log

    def __getattr__(self, name):
        f = getattr(self._mod, name)
        if not callable(f) or isinstance(f, type):
            return f

        def call(*args, **kwargs):
            ts = [a for a in list(args) + list(kwargs.values()) if torch.is_tensor(a)]
            self._log.append("%s(%s)" % (name, " ".join("x".join(map(str, t.shape)) for t in ts)))
            return f(*args, **kwargs)
        return call


def trace(name: str, hw: int, batch: int, device: torch.device):
    torch.manual_seed(0)
    model, _opt, step, _ = build_training(name, 40, device, World(), 4e-4)
    x = (torch.randn(batch, hw, hw, 3) * 0.5).to(device)
    y = torch.randint(0, 40, (batch,)).to(device)
    log, real = [], Fn.K
    Fn.K = lambda t: Traced(real(t), log)
    try:
        step(x.to(torch.bfloat16) if device.type == "cuda" else x, y)
    finally:
        Fn.K = real
    if device.type == "cuda":
        torch.cuda.synchronize()
    grad = model._mpa_arena.grad.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
    return log, hashlib.sha256(grad).hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="+", help="model@image-size, e.g. resnet18@64")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--out", default="", help="directory for the full logs (<model>.trace)")
    a = ap.parse_args()
    for spec in a.models:
        name, hw = spec.split("@")
        log, grad = trace(name, int(hw), a.batch, torch.device(a.device))
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name + ".trace"), "w") as f:
                f.write("\n".join(log) + "\n")
        print("%-12s calls %4d  trace %s  grad %s" % (
            spec, len(log), hashlib.sha256("\n".join(log).encode()).hexdigest()[:16], grad[:16]),
            flush=True)

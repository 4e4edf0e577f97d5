#!/usr/bin/env python3
"""SHA-256 of what the ResNet-50 trunk computes and of the C-ABI calls it makes, route by route, on fixed seeded inputs: one line
`<route> <item> <digest>` per item, and a last line with the number of lines and the digest of all of them.
    python tools/trunk_digest.py [--out FILE]
A refactor of the host code that launches the trunk (egohmr_amd/encoders.py FoldedTrunk, egohmr_amd/trunk_grad.py) is checked this way: the tool uses
only m.folded(**kw)(img), m(img), m.current()(img, saved=acts), trunk_grad.train_forward(m, img) and .backward(gout), so the same file runs in a
checkout from before the change.  Run it twice there, in two processes, and once on the new tree: every line the old tree reproduces against itself
must be equal on the new one (docs/EXPERIMENTS.md R31.1).

Inputs: tests/trunk_grad_ref.make_state / make_image / make_cotangent at (2, 64, 64), seed 2 - the smallest shape at which layer 4 has two rows per
channel.  Routes:
    eval_x2 / eval_two_launch / eval_nhwc / eval_hi_only   folded(), folded(fuse_shortcut=False), folded(x2_activations=False), hi_only = True: output
    eval_module                                            m(img) through current(): output
    eval_grad                                              current()(img, saved=acts): output and every saved X2 buffer; m(img).backward(gout) with
                                                           grad_params: every parameter's gradient
    train                                                  train_batchnorm under .train(), no graph: output, every running statistic and counter
    train_record                                           trunk_grad.train_forward: output, every saved X2 buffer, every running statistic and counter
    train_grad                                             m(img).backward(gout) with grad_params: output, gradients, running statistics and counters
Per route a line `<route> calls <digest>`: the sequence of entry points called through `_lib.api()` with their scalar arguments and the scalar fields
of the descriptors they are handed (pointers count as present / absent) - the recorder of tests/test_gpu_trunk_walk.py."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from egohmr_amd import _lib, trunk_grad  # noqa: E402
from tests import trunk_grad_ref as R  # noqa: E402
from tests import trunk_train_ref as T  # noqa: E402

SHAPE, SEED = (2, 64, 64), 2
LINES, CALLS = [], []


def scalar(a):
    if a is None or isinstance(a, (int, float)):
        return a
    d = getattr(a, "_obj", a)                               # C.byref(descriptor)
    if isinstance(d, C.Structure):
        return tuple((n, ("ptr" if getattr(d, n) is not None else None) if t is C.c_void_p else getattr(d, n))
                     for n, t in d._fields_ if t in (C.c_void_p, C.c_int, C.c_int64, C.c_float))
    return "ptr"


def record():
    A = _lib.api()
    for name, fn in list(vars(A).items()):
        def call(*args, _fn=fn, _name=name):
            CALLS.append((_name, tuple(scalar(a) for a in args)))
            return _fn(*args)
        setattr(A, name, call)


def emit(route, item, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    LINES.append(f"{route} {item} {h.hexdigest()}")
    print(LINES[-1], flush=True)


def emit_calls(route):
    torch.cuda.synchronize()
    LINES.append(f"{route} calls {hashlib.sha256(repr(CALLS).encode()).hexdigest()}")
    print(LINES[-1], f"({len(CALLS)} calls)", flush=True)
    del CALLS[:]


def emit_acts(route, acts):
    for i, (buf, (N, H, W)) in enumerate(acts):            # (the rows behind the N H W pixels pad the row tile: no kernel owes them a value)
        emit(route, f"act{i:02d}_{N}x{H}x{W}", buf[:N * H * W])


def emit_grads(route, m):
    for n, p in m.named_parameters():
        emit(route, "grad:" + n, p.grad)


def emit_stats(route, m):
    for n, b in m.named_buffers():
        emit(route, "buffer:" + n, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    B, H, W = SHAPE
    sd = R.make_state(SEED)
    img, gout = R.make_image(B, H, W, SEED).float().to(dev), R.make_cotangent(B, SEED).float().to(dev)
    record()

    m = R.load_module(sd, dev)
    for route, kw, hi_only in (("eval_x2", {}, False), ("eval_two_launch", dict(fuse_shortcut=False), False),
                               ("eval_nhwc", dict(x2_activations=False), False), ("eval_hi_only", {}, True)):
        m.hi_only = hi_only
        emit(route, "out", m.folded(**kw)(img))
        emit_calls(route)
    m.hi_only = False
    with torch.no_grad():
        emit("eval_module", "out", m(img))
    emit_calls("eval_module")

    m = R.load_module(sd, dev)
    acts = []
    emit("eval_grad", "out", m.current()(img, saved=acts))
    emit_acts("eval_grad", acts)
    m.grad_params = True
    m(img).backward(gout)
    emit_grads("eval_grad", m)
    emit_calls("eval_grad")

    m = T.load_module(sd, dev)
    with torch.no_grad():
        emit("train", "out", m(img))
    emit_stats("train", m)
    emit_calls("train")

    m = T.load_module(sd, dev)
    out, rec = trunk_grad.train_forward(m, img)
    emit("train_record", "out", out)
    emit_acts("train_record", rec.acts)
    emit_stats("train_record", m)
    emit_calls("train_record")

    m = T.load_module(sd, dev)
    m.grad_params = True
    out = m(img)
    out.backward(gout)
    emit("train_grad", "out", out)
    emit_grads("train_grad", m)
    emit_stats("train_grad", m)
    emit_calls("train_grad")

    LINES.append(f"lines {len(LINES)} sha256 {hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
    print(LINES[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

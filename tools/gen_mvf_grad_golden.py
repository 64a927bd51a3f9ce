#!/usr/bin/env python3
"""Writes tests/golden/mvf_bilinear_grad.npz by RUNNING THE REFERENCE's SingleView.bilinear_interpolate (det3d/models/readers/mvf_encoder.py,
imported unmodified) under autograd on the CPU.  Build machine only (needs the reference tree, numpy and torch; no GPU):

    python tools/gen_mvf_grad_golden.py --reference <reference tree>

Inputs: `bil_image` (2, 6, 9, 11) and `bil_coords` (200 rows [b, x, y], positions from -1 to 12 against an 11 x 9 map: points outside on every
side, so the reference's rule of weighting with the CLAMPED corners gives negative weights and coincident corners) of tests/golden/mvf_parts.npz,
and a seeded upstream gradient.  The fixture holds that gradient and the reference's gradient of the map, arrays only.

The reference file imports spconv and torch_scatter at module level; neither is needed by the function called here.  The stand-ins below only
let the file import (the shape of oracle/gen_golden.py's install_spconv_import_stub): nothing of them executes."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def install_import_stand_ins():
    class _Never(torch.nn.Module):
        def __init__(self, *a, **k):
            raise RuntimeError("stand-in: import only")

    sp, spt, core, ts = (types.ModuleType(n) for n in ("spconv", "spconv.pytorch", "spconv.core", "torch_scatter"))
    spt.SparseModule = torch.nn.Module
    spt.SparseSequential = torch.nn.Sequential
    spt.SubMConv2d = spt.SparseConv2d = spt.SubMConv3d = spt.SparseConv3d = spt.SparseConvTensor = _Never
    core.ConvAlgo = types.SimpleNamespace(Native=0)
    sp.pytorch, sp.core = spt, core

    def never(*a, **k):
        raise RuntimeError("stand-in: import only")

    ts.scatter_max = ts.scatter_mean = ts.scatter_add = ts.scatter = never
    for m in (sp, spt, core, ts):
        sys.modules[m.__name__] = m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mvf_bilinear_grad.npz"))
    a = ap.parse_args()
    install_import_stand_ins()
    sys.path.insert(0, a.reference)          # the reference's det3d package, ahead of this repository's alias package of the same name
    for k in [k for k in sys.modules if k == "det3d" or k.startswith("det3d.")]:
        del sys.modules[k]
    from det3d.models.readers.mvf_encoder import SingleView

    assert os.path.realpath(sys.modules[SingleView.__module__].__file__).startswith(os.path.realpath(a.reference)), "not the reference's file"
    parts = np.load(os.path.join(ROOT, "tests", "golden", "mvf_parts.npz"))
    image = torch.from_numpy(parts["bil_image"]).requires_grad_(True)
    coords = torch.from_numpy(parts["bil_coords"])
    out = SingleView.bilinear_interpolate(None, image, coords)
    assert np.array_equal(out.detach().numpy(), parts["bil_out"]), "forward differs from the committed fixture"
    grad_out = torch.from_numpy(np.random.default_rng(20261).standard_normal(tuple(out.shape)).astype(np.float32))
    out.backward(grad_out)
    np.savez_compressed(a.out, grad_out=grad_out.numpy(), grad_image=image.grad.numpy())
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, grad_out {tuple(grad_out.shape)}, grad_image {tuple(image.grad.shape)} "
          f"(torch {torch.__version__}, numpy {np.__version__})")


if __name__ == "__main__":
    main()

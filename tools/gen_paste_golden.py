#!/usr/bin/env python3
"""Writes tests/golden/paste_augment_small.npz by RUNNING THE REFERENCE's augmentation.py (Rotation, Scaling, Translation, Flip with
box_np_ops.py's flip / scaling / rotate / translate / yaw_rotation) and sample_ops.py's BatchSampler on fixed inputs.  Build machine only
(needs the reference tree and numpy; no GPU, no torch):

    python tools/gen_paste_golden.py --reference <reference tree>

The files are loaded by path.  augmentation.py and sample_ops.py import `det3d.core.bbox.box_np_ops` by its absolute name, so stand-in packages of
that name are registered for the duration of the load (and removed again: this repository has a det3d package of its own), and box_np_ops
imports numba, which the build machine need not have: a stand-in module whose decorators return the function unchanged takes its place.  That
is safe for everything recorded here, which is plain numpy.  It is NOT safe for box_collision_test and points_in_boxes_jit: they rely on
numba's value semantics for `is True` / `is False` (in plain Python `np.bool_ is True` is False, which silently skips the containment branch),
so they are never run un-jitted for a fixture; for those two the fp64 statement (tests/paste_augment_ref.py) is the reference.

Nothing of the reference's text is stored; the fixture holds inputs, seeds, the values np.random handed out, and outputs.

Cases: 4000 fp32 points and 48 fp32 boxes (9 columns; row 5 has a NaN vx, row 11 a NaN (vx, vy); yaws reach beyond +-pi so that the flip wrap
fires) inside the 19.2 m x 16 m range of tests/golden/assign_small.npz.  For each seed the four stages run in the YAML's order (rotation,
scaling, translation, flip) on one `res` dict, and the points / boxes are recorded after every stage.  Seed 0 records all points, the other
seeds the first 400 (the boxes are always complete); the last case uses the 7-column boxes.  The flip probabilities are (0.5, 0.5), so the
seeds cover flip x, flip y, both and neither."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 2, 3, 4, 5, 6]
N_SMALL = 400
ROT_RANGE, SCALE_RANGE, TRANS_NOISE, FLIP_PROB = [-0.78539816, 0.78539816], [0.9, 1.1], 0.5, [0.5, 0.5]
SAMPLER_CASES = [(11, 37, [5, 9, 0, 12, 11, 3, 30, 8]), (12, 8, [3, 3, 2, 8, 1, 9]), (13, 1, [1, 1, 2])]   # (seed, list length, the sample() calls)


def load_reference(ref):
    numba = types.ModuleType("numba")
    deco = lambda *a, **k: a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f)  # noqa: E731
    numba.njit = numba.jit = deco
    names = ["det3d", "det3d.core", "det3d.core.bbox", "det3d.core.bbox.box_np_ops", "numba"]
    saved = {n: sys.modules.get(n) for n in names}
    try:
        sys.modules["numba"] = numba
        pkgs = []
        for n in names[:3]:
            m = types.ModuleType(n)
            m.__path__ = []
            sys.modules[n] = m
            pkgs.append(m)
        pkgs[0].core, pkgs[1].bbox = pkgs[1], pkgs[2]

        def load(modname, rel):
            spec = importlib.util.spec_from_file_location(modname, os.path.join(ref, *rel))
            m = importlib.util.module_from_spec(spec)
            sys.modules[modname] = m
            spec.loader.exec_module(m)
            return m

        ops = load("det3d.core.bbox.box_np_ops", ("det3d", "core", "bbox", "box_np_ops.py"))
        pkgs[2].box_np_ops = ops
        aug = load("pnx_ref_augmentation", ("det3d", "datasets", "pipelines", "augmentation.py"))
        smp = load("pnx_ref_sample_ops", ("det3d", "datasets", "pipelines", "sample_ops.py"))
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return aug, smp


def make_inputs():
    rng = np.random.default_rng(31337)
    n, m = 4000, 48
    pts = np.empty((n, 3), np.float32)
    pts[:, 0] = rng.uniform(-9.6, 9.6, n)
    pts[:, 1] = rng.uniform(-8.0, 8.0, n)
    pts[:, 2] = rng.uniform(-5.0, 3.0, n)
    b = np.zeros((m, 9), np.float32)
    b[:, 0] = rng.uniform(-8.5, 8.5, m)
    b[:, 1] = rng.uniform(-7.0, 7.0, m)
    b[:, 2] = rng.uniform(-2.0, 1.0, m)
    b[:, 3:6] = np.exp(rng.uniform(-1.0, 1.2, (m, 3)))
    b[:, 6:8] = rng.normal(0, 2.0, (m, 2))
    b[:, 8] = rng.uniform(-3.6, 3.6, m)
    b[0, 8], b[1, 8], b[2, 8], b[3, 8] = np.pi, -np.pi, 3.1, -3.1     # the wrap's own neighbourhood (fp32(pi) > pi)
    b[5, 6] = np.nan
    b[11, 6:8] = np.nan
    cls = rng.integers(0, 5, m).astype(np.int32)
    return pts, b, cls


class Recorder:
    """np.random.uniform / normal / choice, recording what they hand out."""

    def __init__(self):
        self.log = []
        self._orig = {k: getattr(np.random, k) for k in ("uniform", "normal", "choice")}

    def __enter__(self):
        for k, f in self._orig.items():
            setattr(np.random, k, (lambda f: lambda *a, **kw: self._rec(f(*a, **kw)))(f))
        return self

    def _rec(self, v):
        self.log.append(float(np.asarray(v).reshape(-1)[0]))
        return v

    def __exit__(self, *exc):
        for k, f in self._orig.items():
            setattr(np.random, k, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "paste_augment_small.npz"))
    a = ap.parse_args()
    aug, smp = load_reference(a.reference)
    pts, boxes, cls = make_inputs()
    out = dict(in_points=pts, in_boxes=boxes, in_classes=cls, seeds=np.asarray(SEEDS, np.int64), n_small=np.int64(N_SMALL),
               cfg_rotation=np.asarray(ROT_RANGE, np.float64), cfg_scale=np.asarray(SCALE_RANGE, np.float64), cfg_noise=np.float64(TRANS_NOISE),
               cfg_flip_prob=np.asarray(FLIP_PROB, np.float64))
    stages = [("rot", aug.Rotation(ROT_RANGE)), ("scale", aug.Scaling(SCALE_RANGE)), ("trans", aug.Translation(TRANS_NOISE)), ("flip", aug.Flip(FLIP_PROB))]
    combos = set()
    for ci, seed in enumerate(SEEDS):
        seven = ci == len(SEEDS) - 1
        p = pts.copy() if ci == 0 else pts[:N_SMALL].copy()
        bx = boxes[:, [0, 1, 2, 3, 4, 5, 8]].copy() if seven else boxes.copy()
        res = {"points": p, "annotations": {"gt_boxes": bx}}
        np.random.seed(seed)
        with Recorder() as rec:
            for name, st in stages:
                res = st(res)
                out[f"c{ci}_points_{name}"] = res["points"].copy()
                out[f"c{ci}_boxes_{name}"] = res["annotations"]["gt_boxes"].copy()
        assert len(rec.log) == 5 and res["points"].dtype == np.float32 and res["annotations"]["gt_boxes"].dtype == np.float32
        out[f"c{ci}_draws"] = np.asarray(rec.log, np.float64)   # angle, scale, translate, flip x (0/1), flip y (0/1)
        combos.add((rec.log[3], rec.log[4]))
    assert len(combos) == 4, f"the seeds cover only the flip combinations {sorted(combos)}"
    for si, (seed, n, calls) in enumerate(SAMPLER_CASES):
        np.random.seed(seed)
        s = smp.BatchSampler(list(range(100, 100 + n)), "x")
        got = [np.asarray(s.sample(k), np.int64) for k in calls]
        out[f"s{si}_cfg"] = np.asarray([seed, n], np.int64)
        out[f"s{si}_calls"] = np.asarray(calls, np.int64)
        out[f"s{si}_lens"] = np.asarray([len(g) for g in got], np.int64)
        out[f"s{si}_items"] = np.concatenate(got)
        assert any(len(g) != k for g, k in zip(got, calls)), "no call wrapped"
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, flip combinations {sorted(combos)} (numpy {np.__version__})")


if __name__ == "__main__":
    main()

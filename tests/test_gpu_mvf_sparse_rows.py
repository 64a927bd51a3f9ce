"""GPU: the MVF view ResNets on sparse rows (SingleView.use_sparse_rows: csrc/sparse3d.hip + pnx_sp3_bilinear_gather) against the fp64 twin of
tests/mvf_view_ref.py (held to the modules by tests/test_mvf_view_ref_cpu.py).

The bar of every numerical comparison: with e(path) = max |path - twin| / max |twin| per tensor, the sparse path must stay within 2 x e(masked-dense
fp32 path of the same modules, the path before this switch existed).  The two fp32 paths add the same terms in different orders, so an equally
good path can land on either side of the other -- hence the factor 2; a wrong tap, a missed row or a wrong statistic is orders of magnitude off.
Both errors are printed.  Integer results (active sets, num_batches_tracked) are compared exactly.

The masked-dense yardstick runs under torch's default backend flags (cudnn.deterministic = False, cudnn.benchmark = False: what a fresh process
trains and evaluates with), set and restored around every run here: another test of the suite leaves cudnn.deterministic = True behind, which
makes MIOpen choose other convolution kernels for the dense path and moved its error by up to 4 x between a run of this file alone and a run of the
whole suite.  Measured on an MI355X, sparse rows / masked dense, error of the sampled output: under the default flags eval 1.02e-6 / 6.38e-7,
1.05e-6 / 7.60e-7 (48-192 widths, pillar / cylinder), 4.61e-7 / 4.74e-7, 4.61e-7 / 3.91e-7 (16-48 widths); training 9.8e-7 / 2.2e-6, 1.14e-6 /
2.13e-6, 1.82e-6 / 2.28e-6, 2.15e-6 / 3.07e-6 -- worst ratio over every tensor 1.60.  With cudnn.deterministic = True the dense path is more accurate
and the rows, whose bits do not change, MISS 2 x its error on the output: eval 1.02e-6 / 2.17e-7, 1.05e-6 / 2.47e-7, 4.61e-7 / 2.05e-7, 4.61e-7 /
2.08e-7 (ratios 4.7, 4.3, 2.3, 2.2); training, cylinder grid, 1.14e-6 / 4.86e-7 and 2.15e-6 / 9.35e-7 (2.4, 2.3); every other tensor held.  The
rows' fp32 chains (pnx_sp3_conv: one chain over all taps and input channels) are longer than those kernels'.

Geometry: a pillar-like grid 64 x 48 and a cylinder-like grid 100 x 36 (halved to 50 / 25 / 13: the odd extent), two frames of synth points."""
import contextlib
import copy
import gc
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
yaml = pytest.importorskip("yaml")
pytestmark = pytest.mark.gpu

import mvf_view_ref as V  # noqa: E402
from conftest import ROOT  # noqa: E402
from sync_replay import Replay  # noqa: E402

WIDE = dict(ds_num_filters=[48, 96, 192, 192], layer_nums=[1, 1, 1, 1], num_filters=[32])
DEEP = dict(ds_num_filters=[16, 32, 48, 48], layer_nums=[2, 2, 2, 2], num_filters=[16])
NETS = {"wide": WIDE, "deep": DEEP}


def _reader(net, seed=0, strides=(1, 2, 2, 2)):
    from pillarnext_amd.mvf_encoder import MVFFeatureNet

    torch.manual_seed(seed)
    n = len(net["ds_num_filters"])
    m = MVFFeatureNet(in_channels=5, voxel_size=[0.5, 0.5, 8.0], pc_range=[-12.0, -16.0, -5.0, 12.0, 16.0, 3.0], cylinder_size=[10.0, 0.08, 20.0],
                      cylinder_range=[-180.0, -5.0, 0.0, 180.0, 3.0, 20.0], num_filters=net["num_filters"], layer_nums=net["layer_nums"],
                      ds_layer_strides=list(strides[:n]), ds_num_filters=net["ds_num_filters"], kernel_size=[3] * n, out_channels=32)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.weight.uniform_(0.5, 1.5), mod.bias.uniform_(-0.3, 0.3), mod.running_mean.uniform_(-0.2, 0.2), mod.running_var.uniform_(0.5, 1.5)
    return m.cuda()


def _points(n=5000, frames=2):
    from pillarnext_amd import synth

    pts = synth.make_batch("C1", frames, "sweep", n=n)
    pts[:, 1:3] *= 0.25          # the C1 disc (51.2 m) onto the 12 x 16 m range; what falls outside exercises the reader's range mask
    return torch.from_numpy(pts).cuda()


_inputs = {}


def _view_inputs(name, which):
    """One view's inputs, computed once: (reader, view, fv (P, C), unq, unq_inv, pos, (H, W), B)."""
    key = (name, which)
    if key not in _inputs:
        m = _reader(NETS[name]).eval()
        pts = _points()
        with torch.no_grad():
            feat, pr, cr, B = m.group_views(pts, 2)
            view, r, size = (m.pillarview, pr, (64, 48)) if which == "pillar" else (m.cylinderview, cr, (100, 36))
            fv = view.cell_features(feat, r["unq_inv"], r["coords"].shape[0])
        assert 4000 <= feat.shape[0] // 2 <= 6000, feat.shape
        _inputs[key] = (m, view, fv.clone(), r["coords"], r["unq_inv"], view._pos_columns(feat).clone(), size, B)
    return _inputs[key]


@contextlib.contextmanager
def _default_backend_flags():
    """torch's default convolution backend flags for the time of a run, whatever an earlier test left behind."""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = False, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def _run(view, sparse, fv, unq, inv, pos, size, B, go=None):
    """view.forward with the cell features replaced by the leaf fv -> (out, fv.grad or None); the caller owns `view` (its buffers move in training)."""
    with _default_backend_flags():
        return _run_view(view, sparse, fv, unq, inv, pos, size, B, go)


def _run_view(view, sparse, fv, unq, inv, pos, size, B, go):
    view.use_sparse_rows(sparse)
    leaf = fv.detach().clone().requires_grad_(go is not None)
    view.cell_features = lambda features, unq_inv, num_cells: leaf
    feat = torch.zeros((pos.shape[0], 20), device="cuda")
    if view.mode == "pillar":
        feat[:, 0:2] = pos
    else:
        feat[:, 10:12] = pos
    out = view(feat, unq, inv, np.array(size), B)
    if go is not None:
        out.backward(go)
    del view.cell_features
    return out.detach(), leaf.grad


def _twin(view, fv, unq, inv, pos, size, B, go=None):
    """The fp64 statement on the CPU: (out, fv grad, parameter grads, buffers after the forward, active sets)."""
    params, buffers = V.tensors_of(view, torch.float64, device="cpu", requires_grad=go is not None)
    leaf = fv.detach().double().cpu().requires_grad_(go is not None)
    cells = V.cell_positions(pos, view.bias, view.voxel_size, int(view.ds_rate)).cpu()
    t = V.view_twin(view, leaf, unq.cpu(), cells, inv.cpu(), B, size[0], size[1], params, buffers)
    if go is not None:
        t["out"].backward(go.double().cpu())
    return t["out"].detach(), leaf.grad, {k: p.grad for k, p in params.items()}, t["buffers"], t["sets"]


def _rel(a, t):
    t = t.to(torch.float64)
    return float((a.detach().double().cpu() - t).abs().max()) / float(t.abs().max())


def _hold(rows, what):
    """rows: [(name, e_sparse, e_dense)].  Prints both, asserts e_sparse <= 2 e_dense with e_dense > 0; returns the worst ratio."""
    worst = 0.0
    for name, es, ed in rows:
        print(f"[{what}] {name}: sparse rows {es:.3g}, masked dense {ed:.3g} of the twin's largest entry (ratio {es / ed if ed else float('inf'):.2f})")
        worst = max(worst, es / ed if ed else float("inf"))
    for name, es, ed in rows:
        assert ed > 0, f"{what}, {name}: the masked-dense path has no error against the twin -- choose other inputs"
        assert es <= 2 * ed, f"{what}, {name}: sparse rows {es:.3g} > 2 x masked dense {ed:.3g}"
    print(f"[{what}] worst ratio {worst:.2f}")
    return worst


# ------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("which", ["pillar", "cylinder"])
@pytest.mark.parametrize("name", ["wide", "deep"])
def test_eval_sets_and_output(name, which):
    _, view, fv, unq, inv, pos, size, B = _view_inputs(name, which)
    view = copy.deepcopy(view).eval()
    t_out, _, _, _, t_sets = _twin(view, fv, unq, inv, pos, size, B)
    with torch.no_grad():
        sets = view.sparse_sets(fv, unq, B, size[0], size[1])
        assert len(sets) == len(t_sets) == 4
        extent = size
        for i, ((coords, x, ix), ts) in enumerate(zip(sets, t_sets)):
            extent = tuple((e + 2 - 3) // view.blocks[i][0].stride + 1 for e in extent)
            assert ix.grid == (1, *extent) and x.shape == (coords.shape[0], view.blocks[i][0].conv.out_channels)
            assert not bool(coords[:, 1].any()) and torch.equal(coords[:, [0, 2, 3]].long().cpu(), ts), f"stage {i}: active set"
            print(f"[{name} {which}] stage {i}: {coords.shape[0]} rows of {B * extent[0] * extent[1]} cells")
        assert extent == ((8, 6) if which == "pillar" else (13, 5))
        sparse, _ = _run(view, True, fv, unq, inv, pos, size, B)
        dense, _ = _run(view, False, fv, unq, inv, pos, size, B)
        again, _ = _run(view, True, fv, unq, inv, pos, size, B)
    assert sparse.shape == dense.shape == (pos.shape[0], view.blocks[-1][0].conv.out_channels)
    assert torch.equal(sparse, again), "eval on rows is not bit-identical run to run"
    _hold([("out", _rel(sparse, t_out), _rel(dense, t_out))], f"eval {name} {which}")


def test_folded_weights_follow_the_parameters():
    _, view, fv, unq, inv, pos, size, B = _view_inputs("deep", "pillar")
    view = copy.deepcopy(view).eval()
    with torch.no_grad():
        a, _ = _run(view, True, fv, unq, inv, pos, size, B)
        cache = view.__dict__["_rows_folded_cache"]
        b, _ = _run(view, True, fv, unq, inv, pos, size, B)
        assert view.__dict__["_rows_folded_cache"] is cache and torch.equal(a, b)
        view.blocks[0][0].norm.bias.add_(0.5)
        c, _ = _run(view, True, fv, unq, inv, pos, size, B)
        d, _ = _run(view, False, fv, unq, inv, pos, size, B)
    assert view.__dict__["_rows_folded_cache"] is not cache and not torch.equal(a, c)
    assert float((c - d).abs().max()) <= 1e-4 * float(d.abs().max())


def test_hip_convs_keep_eval_and_rows_take_the_rest():
    """Both switches set: eval under no_grad stays on the 16-bit masked kernels, a call that wants a gradient takes the rows."""
    _, view, fv, unq, inv, pos, size, B = _view_inputs("wide", "pillar")
    view = copy.deepcopy(view).eval().use_hip_convs(torch.bfloat16)
    with torch.no_grad():
        both, _ = _run(view, True, fv, unq, inv, pos, size, B)
        assert view.__dict__.get("_hip_net")
        only16, _ = _run(view, False, fv, unq, inv, pos, size, B)
    assert torch.equal(both, only16)
    go = torch.ones((pos.shape[0], 192), device="cuda")
    out, g = _run(view, True, fv, unq, inv, pos, size, B, go)              # eval mode, gradients wanted: rows, norms on their running statistics
    ref, gref = _run(view.use_hip_convs(None), False, fv, unq, inv, pos, size, B, go)
    assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) and float((g - gref).abs().max()) <= 1e-4 * float(gref.abs().max())


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("which", ["pillar", "cylinder"])
@pytest.mark.parametrize("name", ["wide", "deep"])
def test_training_step_against_the_twin(name, which):
    _, view0, fv, unq, inv, pos, size, B = _view_inputs(name, which)
    view0 = copy.deepcopy(view0).train()
    gen = torch.Generator(device="cuda").manual_seed(7)
    go = torch.randn((pos.shape[0], view0.blocks[-1][0].conv.out_channels), device="cuda", generator=gen)
    t_out, t_gfv, t_gp, t_buf, _ = _twin(view0, fv, unq, inv, pos, size, B, go)
    res = {}
    for sparse in (True, False):
        view = copy.deepcopy(view0)
        out, gfv = _run(view, sparse, fv, unq, inv, pos, size, B, go)
        res[sparse] = (out, gfv, {k: p.grad for k, p in view.blocks.named_parameters()}, dict(view.blocks.named_buffers()))
    rows = [("out", _rel(res[True][0], t_out), _rel(res[False][0], t_out)), ("d fv", _rel(res[True][1], t_gfv), _rel(res[False][1], t_gfv))]
    for k in t_gp:
        assert res[True][2][k] is not None and res[True][2][k].shape == t_gp[k].shape, k
        rows.append((f"d {k}", _rel(res[True][2][k], t_gp[k]), _rel(res[False][2][k], t_gp[k])))
    for k, v in t_buf.items():
        if v.dtype == torch.int64:
            assert int(res[True][3][k]) == int(v) == int(res[False][3][k]), k
        else:
            rows.append((k, _rel(res[True][3][k], v), _rel(res[False][3][k], v)))
    _hold(rows, f"train {name} {which}")


# ------------------------------------------------------------------------------------------------ edge inputs
def test_second_frame_empty_keeps_its_slot():
    """batch_size=2 with points in frame 0 only: the index covers both frames, every stage's rows lie in frame 0, both views agree with the
    masked-dense path (1e-4 of the largest entry: fp32 order, two BatchNorm'd stacks apart), the reader's map keeps an all-zero frame 1.  The
    reader's own output is not compared element by element: its last scatter keeps one of several pillars per coarse cell, whichever (mvf:322-327)."""
    m, *_ = _view_inputs("deep", "pillar")
    pts = _points()
    pts = pts[pts[:, 0] == 0]
    for mode in ("eval", "train"):
        net = copy.deepcopy(m).train(mode == "train")
        with torch.no_grad():
            feat, pr, cr, B = net.group_views(pts, 2)
        assert B == 2
        for view, r, size in ((net.pillarview, pr, (64, 48)), (net.cylinderview, cr, (100, 36))):
            with torch.no_grad():
                fv = view.cell_features(feat, r["unq_inv"], r["coords"].shape[0]) if mode == "eval" else torch.randn((r["coords"].shape[0], 16), device="cuda")
                for coords, _, ix in view.sparse_sets(fv, r["coords"], 2, *size, differentiable=False):
                    assert ix.batch == 2 and coords.shape[0] > 0 and not bool(coords[:, 0].any())
            go = torch.randn((feat.shape[0], 48), device="cuda") if mode == "train" else None
            pos = view._pos_columns(feat)
            with torch.set_grad_enabled(mode == "train"):
                a, ga = _run(copy.deepcopy(view), True, fv, r["coords"], r["unq_inv"], pos, size, 2, go)
                b, gb = _run(copy.deepcopy(view), False, fv, r["coords"], r["unq_inv"], pos, size, 2, go)
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), (mode, view.mode)
            if go is not None:
                assert float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max()), (mode, view.mode)
        with torch.set_grad_enabled(mode == "train"):
            out = net.use_sparse_rows()(pts, batch_size=2)
        assert out.shape == (2, 32, 8, 6) and bool(torch.isfinite(out).all()) and bool(out[0].any()) and not bool(out[1].any())


def test_empty_cloud():
    _, view, fv, unq, inv, pos, size, B = _view_inputs("deep", "cylinder")
    for mode in ("eval", "train"):
        v = copy.deepcopy(view).train(mode == "train")
        go = torch.zeros((0, 48), device="cuda") if mode == "train" else None
        with torch.set_grad_enabled(mode == "train"):
            out, g = _run(v, True, fv[:0], unq[:0], inv[:0], pos[:0], size, B, go)
        assert out.shape == (0, 48) and (g is None or g.shape == fv[:0].shape)
        sets = v.sparse_sets(fv[:0], unq[:0], B, size[0], size[1])
        assert [s[0].shape[0] for s in sets] == [0, 0, 0, 0] and sets[-1][2].grid == (1, 13, 5)
        for k, b in v.blocks.named_buffers():                      # no rows: the running statistics stay where they were
            assert torch.equal(b, dict(view.blocks.named_buffers())[k]), k


def test_one_cell():
    """Every point in one cell.  A stride-2 entry convolution maps a cell with even coordinates onto exactly one output cell: eval agrees with the
    masked-dense path; in training the first norm sees one row and raises as torch's BatchNorm does."""
    view = _reader(dict(ds_num_filters=[16], layer_nums=[1], num_filters=[16]), strides=(2,)).pillarview
    n, size, B = 50, (64, 48), 2
    unq = torch.tensor([[1, 10, 20]], dtype=torch.int32, device="cuda")
    inv = torch.zeros((n,), dtype=torch.int64, device="cuda")
    fv = torch.randn((1, 16), device="cuda")
    centre = torch.tensor(view.bias, dtype=torch.float32) + torch.tensor([20.5, 10.5]) * torch.tensor(view.voxel_size, dtype=torch.float32)
    pos = (centre + (torch.rand((n, 2)) - 0.5) * 0.4).cuda()
    view.eval()
    with torch.no_grad():
        sets = view.sparse_sets(fv, unq, B, *size)
        assert sets[0][0].tolist() == [[1, 0, 5, 10]]
        a, _ = _run(view, True, fv, unq, inv, pos, size, B)
        b, _ = _run(view, False, fv, unq, inv, pos, size, B)
    assert bool(b.any()) and float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    view.train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _run(view, True, fv, unq, inv, pos, size, B, torch.ones((n, 16), device="cuda"))


# ------------------------------------------------------------------------------------------------ synchronised statistics
def test_two_ranks_see_the_joint_batch():
    """models.convert_sync_batchnorm, then two replayed ranks with one frame each against one process with both frames.  Every difference is fp32
    summation order (the ranks' fp64 sums are added across ranks instead of one sum over all rows): 1e-5 of the tensor's largest entry, three
    orders above one fp32 rounding and four below the effect of per-rank statistics."""
    from pillarnext_amd.models import convert_sync_batchnorm

    net = dict(ds_num_filters=[16], layer_nums=[1], num_filters=[16])
    m = _reader(net, strides=(2,)).train()
    pts = _points(3000)
    with torch.no_grad():
        feat, pr, _, B = m.group_views(pts, 2)
        unq, inv = pr["coords"], pr["unq_inv"]
        fv = torch.randn((unq.shape[0], 16), device="cuda")
    pos, size = m.pillarview._pos_columns(feat).clone(), (64, 48)
    go = torch.randn((pos.shape[0], 16), device="cuda")
    p0 = int((unq[:, 0] == 0).sum())                       # unq is sorted [b, y, x]: frame 0's cells are its first p0 rows
    assert 0 < p0 < unq.shape[0] and bool((unq[p0:, 0] == 1).all())
    frame = unq[inv, 0].long()
    idx = [(frame == r).nonzero()[:, 0] for r in (0, 1)]   # the points of each frame

    def step(view, rows, pts_of, shift, batch):
        u = unq[rows].clone()
        u[:, 0] -= shift
        out, g = _run(view, True, fv[rows], u, inv[pts_of] - rows.start, pos[pts_of].contiguous(), size, batch, go[pts_of].contiguous())
        return out, g, {k: p.grad for k, p in view.blocks.named_parameters()}, {k: b.clone() for k, b in view.blocks.named_buffers()}

    joint = step(copy.deepcopy(m.pillarview), slice(0, unq.shape[0]), torch.arange(pos.shape[0], device="cuda"), 0, 2)

    def rank(r, token):
        view = convert_sync_batchnorm(copy.deepcopy(m.pillarview), process_group=token)
        assert view.blocks[0][0].norm.sync and view.blocks[0][0].norm.sync_group is token
        return step(view, slice(0, p0) if r == 0 else slice(p0, unq.shape[0]), idx[r], r, 1)

    rp = Replay(2)
    a, b = rp.run(rank)
    assert rp.passes == 7, "three norms: three collectives forward, three backward"

    def close(x, y, what):
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max()), (what, float((x - y).abs().max()), float(y.abs().max()))

    close(a[0], joint[0][idx[0]], "out, rank 0")
    close(b[0], joint[0][idx[1]], "out, rank 1")
    close(torch.cat([a[1], b[1]]), joint[1], "d fv")
    for k in joint[2]:
        close(a[2][k] + b[2][k], joint[2][k], f"d {k}")
    for k, v in joint[3].items():
        for r in (a, b):
            if v.dtype == torch.int64:
                assert int(r[3][k]) == int(v)
            else:
                close(r[3][k], v, k)


# ------------------------------------------------------------------------------------------------ no canvas
def test_no_map_of_the_grid_is_allocated():
    """A 1024 x 1024 view, 3 000 points, 48 channels at stage 0: everything this test allocates -- the reader, the points, the grouping, forward +
    backward -- stays below the bytes of ONE dense stage-0 activation.  Counted from the start of the test: what earlier tests of the process still
    hold (about 1 GiB in a run of the whole suite) is not this path's."""
    from pillarnext_amd import synth
    from pillarnext_amd.mvf_encoder import MVFFeatureNet

    gc.collect()
    torch.cuda.synchronize()
    start = torch.cuda.memory_allocated()
    torch.manual_seed(0)
    m = MVFFeatureNet(in_channels=5, voxel_size=[0.1, 0.1, 8.0], pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], cylinder_size=[10.0, 0.08, 60.0],
                      cylinder_range=[-180.0, -5.0, 0.0, 180.0, 3.0, 60.0], num_filters=[32], layer_nums=[1, 1, 1, 1], ds_layer_strides=[1, 2, 2, 2],
                      ds_num_filters=[48, 96, 192, 192], kernel_size=[3, 3, 3, 3], out_channels=32).cuda().train()
    pts = torch.from_numpy(synth.make_batch("C1", 2, "sweep", n=1500)).cuda()
    B = 2
    with torch.no_grad():
        feat, pr, _, _ = m.group_views(pts, B)
    assert 2500 <= feat.shape[0] <= 3000
    view = m.pillarview.use_sparse_rows()
    one_map = B * 1024 * 1024 * 48 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = view(feat, pr["coords"], pr["unq_inv"], np.array([1024, 1024]), B)
    out.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"[no canvas] peak {(peak - start) / 2**20:.1f} MiB above the start of the test ({(peak - base) / 2**20:.1f} MiB above the reader and its "
          f"inputs; the process holds {start / 2**20:.1f} MiB from before), one dense stage-0 activation {one_map / 2**20:.1f} MiB")
    assert out.shape == (feat.shape[0], 192) and peak - start < one_map
    assert all(p.grad is not None and bool(p.grad.any()) for p in view.blocks.parameters())


# ------------------------------------------------------------------------------------------------ the detector
def _small_mvf18():
    """The small mvf18 of tests/test_gpu_mvf_train.py."""
    from pillarnext_amd import config

    with open(os.path.join(ROOT, "configs", "mvf18_aspp_waymo.yaml")) as f:
        cfg = yaml.safe_load(f)
    r = cfg["model"]["reader"]
    r["pc_range"], r["voxel_size"] = [-25.6, -25.6, -10.0, 25.6, 25.6, 10.0], [0.1, 0.1, 20]
    r["cylinder_size"], r["cylinder_range"] = [0.703125, 0.4, 40], [-180, -10.0, 0, 180, 10.0, 40]
    r["layer_nums"] = [1, 1, 1, 1]
    pp = cfg["model"]["post_processing"]
    pp["post_center_limit_range"], pp["score_threshold"] = [-30.0, -30.0, -10.0, 30.0, 30.0, 10.0], 0.0
    return config.resolve(cfg)


def _labels(tasks, B, M, H, W, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ex = {"hm": [], "ind": [], "mask": [], "cat": [], "anno_box": [], "gt_boxes": []}
    for names in tasks:
        ex["hm"].append(torch.rand((B, len(names), H, W), device="cuda", generator=gen) * 0.2)
        ex["ind"].append(torch.randint(0, H * W, (B, M), device="cuda", generator=gen))
        mk = torch.zeros((B, M), dtype=torch.uint8, device="cuda")
        mk[:, :6] = 1
        ex["mask"].append(mk)
        ex["cat"].append(torch.randint(0, len(names), (B, M), device="cuda", generator=gen))
        ex["anno_box"].append(torch.randn((B, M, 10), device="cuda", generator=gen) * 0.3)
        ex["gt_boxes"].append(torch.rand((B, M, 7), device="cuda", generator=gen) + torch.tensor([0, 0, -1, 1.5, 0.6, 1.2, 0], device="cuda"))
    return ex


def test_mvf18_detector_training_step_on_rows():
    from pillarnext_amd import config, synth

    cfg = _small_mvf18()
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().train()
    dense = copy.deepcopy(det)
    assert det.reader.use_sparse_rows() is det.reader
    B, M = 2, 16
    H = W = 512 // cfg["_out_size_factor"][0]
    pts = torch.from_numpy(synth.make_batch("C1", B, "sweep", n=6000)).cuda()
    ex = {"points": pts, "batch_size": B, **_labels([list(t) for t in cfg["_tasks"]], B, M, H, W)}
    losses = {}
    for name, d in (("rows", det), ("dense", dense)):
        loss, _ = d(ex)
        assert bool(torch.isfinite(loss)), name
        loss.backward()
        losses[name] = float(loss)
    print(f"[mvf18 on rows] loss {losses['rows']:.6f}, masked dense {losses['dense']:.6f}")
    for view in ("pillarview", "cylinderview"):
        ref = dict(getattr(dense.reader, view).blocks.named_parameters())
        for k, p in getattr(det.reader, view).blocks.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), f"reader.{view}.blocks.{k}"
            print(f"[mvf18 on rows] reader.{view}.blocks.{k}: relative difference to the masked-dense step "
                  f"{float((p.grad - ref[k].grad).abs().max()) / max(float(ref[k].grad.abs().max()), 1e-30):.3g}")

"""GPU: the multi-view reader's per-point layers on the fused training node (PNX_TRAIN_POINT_HIP; ops.PointLayer on csrc/point_layer_train.hip) --
the wiring.  The small MVFFeatureNet of test_gpu_mvf_train.py::test_single_view_trains_on_the_node (4000 points, 2 frames): one forward + backward
with the switch on and off, on the same weights and the same upstream gradient; the node runs exactly where the switch says (grad_fn names), the
outputs agree to 1e-5 absolute (the bound that file uses between two paths), every parameter gradient of the PFN layers and the PointNets agrees per
tensor to 2 * 2^-16 * max |g| (each path is within the bar of the same fp64 value, tests/point_layer_ref.py); the running statistics of all six
norms advance once per forward under both settings; pointnet2 writes no per-point tensor; eval() is untouched; a SyncBatchNorm takes the node in
a world of one process and torch in a larger one; the small mvf18 detector still takes a finite, changing training step with the node on."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SWITCH = "PNX_TRAIN_POINT_HIP"
NORMS = ("pillarview.pfn_layers.0", "pillarview.pfn_layers.1", "cylinderview.pfn_layers.0", "cylinderview.pfn_layers.1", "pointnet1", "pointnet2")


def _small_reader(layer_nums=(1, 1)):
    from pillarnext_amd.mvf_encoder import MVFFeatureNet

    torch.manual_seed(2)
    pr, vs = [-25.6, -25.6, -10.0, 25.6, 25.6, 10.0], [0.2, 0.2, 20]
    return MVFFeatureNet(in_channels=5, voxel_size=vs, pc_range=pr, cylinder_size=[1.40625, 0.4, 40], cylinder_range=[-180, -10.0, 0, 180, 10.0, 40],
                         num_filters=[16, 16], layer_nums=list(layer_nums), ds_layer_strides=[1, 2], ds_num_filters=[16, 32], kernel_size=[3, 3],
                         out_channels=64).cuda().train()


def _points(n=4000):
    from pillarnext_amd import synth

    return torch.from_numpy(synth.make_batch("C1", 2, "sweep", n=n)).cuda()


def _pillars(m, pts, B=2):
    """MVFFeatureNet.forward up to the per-pillar maximum (P, C).  The dense map behind it keeps ONE of the pillars that share a coarse cell, which
    one is unspecified (index_put without accumulate): two runs of the same path differ there, so the paths are compared in front of it."""
    feat, pr, cr, B = m.group_views(pts, B)
    from pillarnext_amd.voxel_encoder import grid_of

    psize = grid_of(m.voxelization.pc_range, m.voxelization.voxel_size)[[1, 0]]
    csize = grid_of(m.cylinderlization.pc_range, m.cylinderlization.voxel_size)[[1, 0]]
    pv = m.pillarview(feat, pr["coords"], pr["unq_inv"], psize, B)
    cv = m.cylinderview(feat, cr["coords"], cr["unq_inv"], csize, B)
    x = torch.cat((m.pointnet1(feat), pv, cv), dim=-1)
    return m.pointnet2.cell_max(x, pr["unq_inv"], pr["coords"].shape[0])


def _grad_fns(t):
    """Names of the autograd nodes below t."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo.extend(g for g, _ in f.next_functions)
    return names


def test_node_against_torch_on_a_small_reader(monkeypatch):
    m = _small_reader()
    pts = _points()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    go, runs = None, {}
    for switch in ("1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        names = _grad_fns(m(pts, batch_size=2))                  # the public forward: where the node runs
        m.load_state_dict(state)                                    # (that forward advanced the running statistics)
        out = _pillars(m, pts)
        assert sorted(n for n in _grad_fns(out) if n in ("PointLayerBackward", "ScatterMaxBackward")) == sorted(n for n in names if n in ("PointLayerBackward", "ScatterMaxBackward"))
        # six per-point layers; with the switch off none of them is the node, and the per-cell maxima are the scatter-max node's
        assert names.count("PointLayerBackward") == (6 if switch == "1" else 0), names.count("PointLayerBackward")
        assert names.count("ScatterMaxBackward") == (0 if switch == "1" else 7), names.count("ScatterMaxBackward")
        if go is None:
            go = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        out.backward(go)
        torch.cuda.synchronize()
        mods = dict(m.named_modules())
        runs[switch] = dict(out=out.detach().clone(), grads={k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                            stats={k: (mods[k].norm.running_mean.clone(), mods[k].norm.running_var.clone(), int(mods[k].norm.num_batches_tracked)) for k in NORMS})
    a, b = runs["1"], runs["0"]
    assert float((a["out"] - b["out"]).abs().max()) <= 1e-5
    keys = [k for k in a["grads"] if k.startswith(tuple(n + "." for n in NORMS))]
    assert len(keys) == 18 and set(a["grads"]) == set(b["grads"])
    for k in keys:
        ga, gb = a["grads"][k], b["grads"][k]
        bound = 2 * 2.0 ** -16 * float(gb.abs().max())
        err = float((ga - gb).abs().max())
        print(f"[mvf point layers] {k}: max |node - torch| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    for k in NORMS:                                                 # momentum 0.01 from the initial (0, 1): moved once, by the same batch statistics
        (rma, rva, na), (rmb, rvb, nb) = a["stats"][k], b["stats"][k]
        assert na == nb == 1 and bool((rva != 1).all()) and bool(rma.any())
        torch.testing.assert_close(rma, rmb, rtol=1e-4, atol=1e-7)
        torch.testing.assert_close(rva, rvb, rtol=1e-5, atol=0)
    # a second forward advances them again
    monkeypatch.setenv(SWITCH, "1")
    m(pts, batch_size=2)
    assert all(int(dict(m.named_modules())[k].norm.num_batches_tracked) == 2 for k in NORMS)
    assert set(m.state_dict()) == set(state)


def test_pointnet2_writes_no_per_point_tensor(monkeypatch):
    m = _small_reader(layer_nums=(0, 0))
    pts = _points(20_000)
    peak = {}
    for switch in ("1", "0", "1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        with torch.no_grad():
            feat, pr, cr, _ = m.group_views(pts, 2)
            x = torch.randn((feat.shape[0], 96), device="cuda")
            torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = m.pointnet2.cell_max(x, pr["unq_inv"], pr["G"])
        torch.cuda.synchronize()
        peak[switch] = torch.cuda.max_memory_allocated() - base
        assert out.shape == (pr["G"], 64) and (type(out.grad_fn).__name__ == "PointLayerBackward") == (switch == "1")
        del out
    n = feat.shape[0]
    assert n > 15_000
    print(f"[mvf point layers] pointnet2 forward at {n} points: peak above the inputs {peak['1'] / 2**20:.2f} MiB on the node, {peak['0'] / 2**20:.2f} MiB on torch")
    assert peak["0"] - peak["1"] >= n * 64 * 4, (peak, n * 64 * 4)


def test_eval_is_untouched(monkeypatch):
    m = _small_reader().eval()
    pts = _points()
    outs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        with torch.no_grad():
            outs[switch] = _pillars(m, pts)
            assert m(pts, batch_size=2).shape[1] == 64
        x = torch.randn((100, 20), device="cuda")
        assert type(m.pointnet1(x).grad_fn).__name__ != "PointLayerBackward"
        assert "PointLayerBackward" not in _grad_fns(m.pointnet2.cell_max(torch.randn((100, 96), device="cuda"), torch.arange(100, device="cuda") // 3, 34))
    torch.testing.assert_close(outs["1"], outs["0"], rtol=0, atol=1e-6)
    assert all(int(dict(m.named_modules())[k].norm.num_batches_tracked) == 0 for k in NORMS)


def test_sync_batchnorm_takes_the_node_only_in_a_world_of_one(monkeypatch):
    from torch import nn

    from pillarnext_amd import ops
    from pillarnext_amd.mvf_encoder import PointNet

    monkeypatch.setenv(SWITCH, "1")
    torch.manual_seed(0)
    pn = PointNet(20, 24).cuda().train()
    ref = PointNet(20, 24).cuda().train()
    ref.load_state_dict(pn.state_dict())
    sync = nn.SyncBatchNorm(24, eps=1e-3, momentum=0.01).cuda().train()
    sync.load_state_dict(pn.norm.state_dict())
    pn.norm = sync
    x = torch.randn((500, 20), device="cuda")
    y = pn(x)
    assert type(y.grad_fn).__name__ == "PointLayerBackward"
    torch.testing.assert_close(y, ref(x), rtol=0, atol=1e-5)
    torch.testing.assert_close(sync.running_var, ref.norm.running_var, rtol=1e-5, atol=0)
    assert int(sync.num_batches_tracked) == 1
    # a world of two (no process group is created, no collective runs: only the routing decision is taken)
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    assert not ops.point_layer_serves(pn, sync)
    assert ops.point_layer_serves(ref, ref.norm)                   # a plain BatchNorm1d keeps the node
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    assert ops.point_layer_serves(pn, sync)
    monkeypatch.setenv(SWITCH, "0")
    assert not ops.point_layer_serves(ref, ref.norm)
    ref.eval()
    monkeypatch.setenv(SWITCH, "1")
    assert not ops.point_layer_serves(ref, ref.norm)


def test_autocast_still_computes_in_fp32(monkeypatch):
    from pillarnext_amd.mvf_encoder import PointNet

    monkeypatch.setenv(SWITCH, "1")
    torch.manual_seed(0)
    pn = PointNet(20, 24).cuda().train()
    x = torch.randn((500, 20), device="cuda")
    y32 = pn(x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = pn(x)
    assert y.dtype == torch.float32 and torch.equal(y, y32)


def test_small_mvf18_training_step_with_the_node(monkeypatch):
    import test_gpu_mvf_train as M
    from pillarnext_amd import config, synth

    monkeypatch.setenv(SWITCH, "1")
    cfg = M._small_mvf18()
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().train()
    B, Mx = 2, 16
    H = W = 512 // cfg["_out_size_factor"][0]
    pts = torch.from_numpy(synth.make_batch("C1", B, "sweep", n=6000)).cuda()
    ex = {"points": pts, "batch_size": B, **M._labels([list(t) for t in cfg["_tasks"]], B, Mx, H, W)}
    opt = torch.optim.SGD(det.parameters(), lr=1e-3)
    loss, _ = det(ex)
    assert bool(torch.isfinite(loss)) and "PointLayerBackward" in _grad_fns(loss)
    opt.zero_grad()
    loss.backward()
    for k, p in det.reader.named_parameters():
        if k.startswith(tuple(n + "." for n in NORMS)):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), k
    opt.step()
    loss2, _ = det(ex)
    print(f"[mvf18 training step, point layers on the node] loss {loss.item():.6f} -> {loss2.item():.6f}")
    assert bool(torch.isfinite(loss2)) and loss2.item() != loss.item()
    assert np.isfinite(loss2.item())

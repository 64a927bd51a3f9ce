"""GPU: the mvf18_aspp detector (configs/mvf18_aspp_waymo.yaml) and the training path of its point sampling -- pnx_bilinear_gather_backward, the
autograd node ops.BilinearGather and SingleView's use of it -- against the fp64 twin of tests/mvf_bilinear_ref.py under its derived bound
|got - S| <= gamma(k + 1) * sum|terms| (one rounding per product, fp32 summation of k terms in any fixed order)."""
import ctypes
import os

import mvf_bilinear_ref as R
import numpy as np
import pytest
import torch
import yaml
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

CELLS4 = [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [2, 0, 0]]      # image indices 0, 1 and, for a 2-image map, -1 and B: the last two contribute nothing


def _raw_backward(go, shape, pos, mn, vs, cells, inv, ds, out, ws):
    """The C entry point with the caller's output and workspace tensors (ops.bilinear_gather_backward allocates its own)."""
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    B, C, H, W = shape
    n = pos.shape[0]
    f2 = lambda v: (ctypes.c_float * 2)(float(v[0]), float(v[1]))  # noqa: E731
    check(lib().pnx_bilinear_gather_backward(ptr(go), go.stride(0) if n > 1 else C, B, H, W, C, ptr(pos), pos.stride(0) if n > 1 else 2, f2(mn), f2(vs),
                                             ptr(cells), ptr(inv), ds, n, ptr(out), ptr(ws), ws.numel(), stream_ptr()), "pnx_bilinear_gather_backward")


def _twin(go, shape, pos, mn, vs, cells, inv, ds):
    b = cells.cpu().numpy()[inv.cpu().numpy(), 0]
    return R.grad_image(go.cpu().numpy(), shape, pos.cpu().numpy(), mn, vs, b, ds)


def _sliced(n, C, gen):
    """(n, C) upstream gradient as a column slice of a wider buffer: row stride C + 7, first column at an odd offset."""
    wide = torch.randn((n, C + 7), device="cuda", generator=gen)
    return wide[:, 3:3 + C]


# ------------------------------------------------------------------------------------------------ 1. the reference's fixture
def test_backward_kernel_on_the_reference_fixture():
    from pillarnext_amd import ops
    from pillarnext_amd._lib import lib

    parts, grad = load_golden("mvf_parts"), load_golden("mvf_bilinear_grad")
    shape = parts["bil_image"].shape
    co = torch.from_numpy(parts["bil_coords"]).cuda()
    go = torch.from_numpy(grad["grad_out"]).cuda()
    cells = torch.tensor(CELLS4[:2], dtype=torch.int32, device="cuda")
    inv = co[:, 0].long().contiguous()
    for pos, mn, vs, ds, what in ((co[:, 1:3], [0.0, 0.0], [1.0, 1.0], 1, "fixture, identity"),
                                  (co[:, 1:3] * 0.5 - 3.0, [-3.0, -3.0], [0.25, 0.25], 2, "fixture, ((pos - min) / voxel) / ds")):
        S, A, k = _twin(go, shape, pos, mn, vs, cells, inv, ds)
        got = ops.bilinear_gather_backward(go, shape, pos, mn, vs, cells, inv, ds)
        assert got.shape == shape and got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
        R.check(got.cpu().numpy(), S, A, k, what)
        # fully written: cells without a term are +0 although the output held NaN
        B, C, H, W = shape
        out = torch.full((B, H, W, C), float("nan"), device="cuda")
        ws = torch.empty(lib().pnx_bilinear_gather_backward_workspace_bytes(pos.shape[0], B, H, W), dtype=torch.uint8, device="cuda")
        _raw_backward(go, shape, pos, mn, vs, cells, inv, ds, out, ws)
        assert torch.equal(out.permute(0, 3, 1, 2), got) and int((k == 0).sum()) > 0
    # the reference's own gradient of the identity case lies under the same bound (tests/test_mvf_bilinear_grad_cpu.py): both bracket S
    S, A, k = _twin(go, shape, co[:, 1:3], [0.0, 0.0], [1.0, 1.0], cells, inv, 1)
    R.check(grad["grad_image"], S, A, k, "reference")


# ------------------------------------------------------------------------------------------------ 2. smallest shapes
def _edge_points(H, W, B, ds, gen):
    """Positions in cell units left, right, above and below the map, at exact integers and in the last row and column, plus random ones; as
    raw positions with min -4 and voxel 0.5 (both exact in fp32, so the integers stay integers)."""
    xs = sorted({-2.5, -1.0, -0.25, 0.0, 0.5, 1.0, W - 1.5, W - 1.0, W - 0.5, float(W), W + 1.5})
    ys = sorted({-2.5, -1.0, -0.25, 0.0, 0.5, 1.0, H - 1.5, H - 1.0, H - 0.5, float(H), H + 1.5})
    u = torch.tensor([[x, y] for x in xs for y in ys], dtype=torch.float32, device="cuda")
    rnd = torch.rand((64, 2), device="cuda", generator=gen) * torch.tensor([W + 3.0, H + 3.0], device="cuda") - 1.5
    u = torch.cat([u, rnd])
    pos = torch.zeros((u.shape[0], 5), device="cuda")
    pos[:, 1:3] = (u * ds) * 0.5 - 4.0
    cells = torch.tensor(CELLS4, dtype=torch.int32, device="cuda")
    inv = (torch.arange(u.shape[0], device="cuda") * 7 % 4).long()       # every image index, -1 and B included, at every kind of position
    return pos[:, 1:3], [-4.0, -4.0], [0.5, 0.5], cells, inv


@pytest.mark.parametrize("ds", [1, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 1), (9, 11)])
def test_backward_kernel_smallest_shapes(H, W, ds):
    from pillarnext_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(100 * H + W + ds)
    B = 2
    pos, mn, vs, cells, inv = _edge_points(H, W, B, ds, gen)
    n = pos.shape[0]
    assert pos.stride(0) == 5
    for C in (1, 48, 64, 65, 192, 200):                                   # lanes are channels: the remainders past 64 and 128, and past one pass of 256
        go = _sliced(n, C, gen)
        assert go.stride(0) == C + 7 and go.storage_offset() == 3
        shape = (B, C, H, W)
        S, A, k = _twin(go, shape, pos, mn, vs, cells, inv, ds)
        assert int(k.sum()) == 4 * int(((inv == 0) | (inv == 1)).sum())  # the points of images -1 and B contribute nothing
        got = ops.bilinear_gather_backward(go, shape, pos, mn, vs, cells, inv, ds)
        R.check(got.cpu().numpy(), S, A, k, f"{H} x {W} map, {C} channels, ds {ds}")
        # n = 0: no launch, a zero-filled gradient
        z = ops.bilinear_gather_backward(go[:0], shape, pos[:0], mn, vs, cells, inv[:0], ds)
        assert z.shape == shape and not bool(z.any()) and not bool(torch.signbit(z).any())


def test_backward_kernel_more_than_256_channels():
    """The channel count is unrestricted: past 256 a cell's points are walked once more per 256 channels."""
    from pillarnext_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(7)
    pos, mn, vs, cells, inv = _edge_points(5, 6, 2, 2, gen)
    for C in (256, 257, 600):
        go = _sliced(pos.shape[0], C, gen)
        S, A, k = _twin(go, (2, C, 5, 6), pos, mn, vs, cells, inv, 2)
        R.check(ops.bilinear_gather_backward(go, (2, C, 5, 6), pos, mn, vs, cells, inv, 2).cpu().numpy(), S, A, k, f"{C} channels")


# ------------------------------------------------------------------------------------------------ 3. one point per cell: the forward's weights, bit for bit
def test_one_point_per_cell_is_one_rounded_product():
    from pillarnext_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(3)
    H, W, C = 8, 10, 70
    base = torch.tensor([[2.0 * i, 2.0 * j] for i in range(W // 2) for j in range(H // 2)], device="cuda")   # base corners two apart: no cell is shared
    u = base + torch.rand(base.shape, device="cuda", generator=gen) * 0.98 + 0.01
    mn, vs, ds = [-1.7, 0.3], [0.3, 0.7], 4                                                                 # a transform that rounds
    pos = (u * ds) * torch.tensor(vs, device="cuda") + torch.tensor(mn, device="cuda")
    n = pos.shape[0]
    cells = torch.tensor([[0, 0, 0]], dtype=torch.int32, device="cuda")
    inv = torch.zeros((n,), dtype=torch.int64, device="cuda")
    go = _sliced(n, C, gen)
    got = ops.bilinear_gather_backward(go, (1, C, H, W), pos, mn, vs, cells, inv, ds).cpu().numpy()
    x0, x1, y0, y1, wa, wb, wc, wd = R.corners_and_weights(pos.cpu().numpy(), mn, vs, ds, H, W)
    g = go.cpu().numpy()
    exp = np.zeros((1, C, H, W), np.float32)
    seen = np.zeros((H, W), np.int64)
    for yy, xx, w in ((y0, x0, wa), (y1, x0, wb), (y0, x1, wc), (y1, x1, wd)):
        assert w.dtype == np.float32 and g.dtype == np.float32
        exp[0][:, yy, xx] = (np.float32(0) + w[:, None] * g).T                    # float32(w) * float32(g), rounded once
        np.add.at(seen, (yy, xx), 1)
    assert seen.max() == 1 and int(seen.sum()) == 4 * n
    assert np.array_equal(got.view(np.int32), exp.view(np.int32))


# ------------------------------------------------------------------------------------------------ 4. + 5. long and uneven segments; determinism
def _long_cases():
    gen = torch.Generator(device="cuda").manual_seed(11)
    one = torch.tensor([[0, 0, 0]], dtype=torch.int32, device="cuda")
    # 5 000 points in one base cell beside empty cells
    pos_a = 1.0 + torch.rand((5000, 2), device="cuda", generator=gen)
    a = (_sliced(5000, 192, gen), (1, 192, 4, 4), pos_a, [0.0, 0.0], [1.0, 1.0], one, torch.zeros((5000,), dtype=torch.int64, device="cuda"), 1)
    # 70 001 points over a 16 x 16 map of 2 images, a few of them outside
    n = 70_001
    pos_b = torch.rand((n, 2), device="cuda", generator=gen) * 18.0 - 1.0
    cells = torch.tensor(CELLS4[:2], dtype=torch.int32, device="cuda")
    b = (_sliced(n, 48, gen), (2, 48, 16, 16), pos_b, [0.0, 0.0], [1.0, 1.0], cells, torch.randint(0, 2, (n,), device="cuda", generator=gen), 1)
    return {"5000 points in one cell": a, "70001 points, 2 x 16 x 16": b}


def test_long_and_uneven_segments_and_determinism():
    from pillarnext_amd import ops

    for what, args in _long_cases().items():
        S, A, k = _twin(*args)
        got = ops.bilinear_gather_backward(*args)
        R.check(got.cpu().numpy(), S, A, k, what)
        if what.startswith("5000"):
            assert int((k > 0).sum()) == 4 and int(k.max()) == 5000 and int((k == 0).sum()) == 12
        # the same inputs give the same bits, also after the workspace was overwritten
        again = ops.bilinear_gather_backward(*args)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), what
        assert ops._BILGRAD_WS.buf is not None
        ops._BILGRAD_WS.buf.fill_(0xFF)
        third = ops.bilinear_gather_backward(*args)
        assert torch.equal(got.view(torch.int32), third.view(torch.int32)), what


# ------------------------------------------------------------------------------------------------ 6. the autograd node and SingleView
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_autograd_node(dtype):
    from pillarnext_amd import ops

    dt = getattr(torch, dtype)
    gen = torch.Generator(device="cuda").manual_seed(5)
    pos, mn, vs, cells, inv = _edge_points(9, 11, 2, 2, gen)
    C = 65
    img = torch.randn((2, C, 9, 11), device="cuda", generator=gen).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = ops.BilinearGather.apply(img, pos, mn, vs, cells, inv, 2)
    assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), ops.bilinear_gather(img.detach(), pos, mn, vs, cells, inv, 2).view(torch.int32))
    wide = torch.randn((pos.shape[0], 3 * C), device="cuda", generator=gen)
    go = wide[:, C:2 * C]
    out.backward(go)
    want = ops.bilinear_gather_backward(go, img.shape, pos, mn, vs, cells, inv, 2).to(dt)
    assert img.grad.dtype == dt and img.grad.shape == img.shape and torch.equal(img.grad, want)
    # an expanded gradient (sum().backward()) is made dense first
    img.grad = None
    ops.BilinearGather.apply(img, pos, mn, vs, cells, inv, 2).sum().backward()
    ones = torch.ones((pos.shape[0], C), device="cuda")
    assert torch.equal(img.grad, ops.bilinear_gather_backward(ones, img.shape, pos, mn, vs, cells, inv, 2).to(dt))


def test_single_view_trains_on_the_node(monkeypatch):
    from pillarnext_amd import synth
    from pillarnext_amd.mvf_encoder import MVFFeatureNet

    torch.manual_seed(2)
    pr, vs = [-25.6, -25.6, -10.0, 25.6, 25.6, 10.0], [0.2, 0.2, 20]
    m = MVFFeatureNet(in_channels=5, voxel_size=vs, pc_range=pr, cylinder_size=[1.40625, 0.4, 40], cylinder_range=[-180, -10.0, 0, 180, 10.0, 40],
                      num_filters=[16, 16], layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[16, 32], kernel_size=[3, 3], out_channels=64).cuda().train()
    pts = torch.from_numpy(synth.make_batch("C1", 2, "sweep", n=4000)).cuda()
    with torch.no_grad():
        feat, rp, rc, _ = m.group_views(pts, 2)
    for view, r, size in ((m.pillarview, rp, (256, 256)), (m.cylinderview, rc, (50, 256))):
        maps = []

        def keep_map(mod, inp, out):                       # the view's map: the last stage's output, with its gradient kept
            out[0].retain_grad()
            maps.append(out[0])

        hook = view.blocks[-1].register_forward_hook(keep_map)
        go = torch.randn((feat.shape[0], 32), device="cuda")
        outs = {}
        for switch in ("1", "0"):
            monkeypatch.setenv("PNX_TRAIN_BILINEAR_HIP", switch)
            out = view(feat, r["coords"], r["unq_inv"], size, 2)
            assert (type(out.grad_fn).__name__ == "BilinearGatherBackward") == (switch == "1"), type(out.grad_fn).__name__
            out.backward(go)
            outs[switch] = out.detach()
        hook.remove()
        assert float((outs["1"] - outs["0"]).abs().max()) <= 1e-5
        x1, x0 = maps
        H, W = x1.shape[2:]
        assert (H, W) == (size[0] // 2, size[1] // 2) and x1.grad is not None and x0.grad is not None
        pos = view._pos_columns(feat)
        S, A, k = _twin(go, tuple(x1.shape), pos, view.bias, view.voxel_size, r["coords"], r["unq_inv"], int(view.ds_rate))
        R.check(x1.grad.cpu().numpy(), S, A, k, f"{view.mode} view, node")
        R.check(x0.grad.cpu().numpy(), S, A, k, f"{view.mode} view, torch statement")
        # positions that need a gradient: the torch statement serves, whatever the switch says
        monkeypatch.setenv("PNX_TRAIN_BILINEAR_HIP", "1")
        fg = feat.clone().requires_grad_(True)
        out = view(fg, r["coords"], r["unq_inv"], size, 2)
        assert type(out.grad_fn).__name__ != "BilinearGatherBackward"
        out.backward(go)
        assert fg.grad is not None and bool(fg.grad[:, :2].any() if view.mode == "pillar" else fg.grad[:, 10:12].any())
        torch.testing.assert_close(out.detach(), outs["0"], rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 7. the detector
def _small_mvf18():
    from pillarnext_amd import config

    with open(os.path.join(ROOT, "configs", "mvf18_aspp_waymo.yaml")) as f:
        cfg = yaml.safe_load(f)
    r = cfg["model"]["reader"]
    r["pc_range"], r["voxel_size"] = [-25.6, -25.6, -10.0, 25.6, 25.6, 10.0], [0.1, 0.1, 20]
    r["cylinder_size"], r["cylinder_range"] = [0.703125, 0.4, 40], [-180, -10.0, 0, 180, 10.0, 40]
    r["layer_nums"] = [1, 1, 1, 1]
    pp = cfg["model"]["post_processing"]
    pp["post_center_limit_range"], pp["score_threshold"] = [-30.0, -30.0, -10.0, 30.0, 30.0, 10.0], 0.0
    cfg = config.resolve(cfg)                      # the head's and the post-processing's geometry follow the reader's through the interpolations
    assert cfg["model"]["head"]["pc_range"] == r["pc_range"] and cfg["model"]["post_processing"]["voxel_size"] == r["voxel_size"]
    return cfg


def _labels(tasks, B, M, H, W, seed=3):
    """Random targets as tests/test_gpu_sparse3d_grad.py builds them for the voxel18 training step."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ex = {"hm": [], "ind": [], "mask": [], "cat": [], "anno_box": [], "gt_boxes": []}
    for names in tasks:
        ex["hm"].append(torch.rand((B, len(names), H, W), device="cuda", generator=gen) * 0.2)
        ex["ind"].append(torch.randint(0, H * W, (B, M), device="cuda", generator=gen))
        m = torch.zeros((B, M), dtype=torch.uint8, device="cuda")
        m[:, :6] = 1
        ex["mask"].append(m)
        ex["cat"].append(torch.randint(0, len(names), (B, M), device="cuda", generator=gen))
        ex["anno_box"].append(torch.randn((B, M, 10), device="cuda", generator=gen) * 0.3)
        ex["gt_boxes"].append(torch.rand((B, M, 7), device="cuda", generator=gen) + torch.tensor([0, 0, -1, 1.5, 0.6, 1.2, 0], device="cuda"))
    return ex


def test_mvf18_detector_end_to_end():
    from pillarnext_amd import config, synth
    from pillarnext_amd.models import SingleStageDetector

    cfg = _small_mvf18()
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().eval()
    assert isinstance(det, SingleStageDetector) and det.backbone is None
    det.reader.use_hip_convs()
    pts = torch.from_numpy(synth.make_batch("C1", 2, "sweep", n=6000)).cuda()
    ex = {"points": pts, "token": ["a", "b"], "batch_size": 2}
    out = det(ex)
    assert set(out) == {"a", "b"}
    for t in out:
        assert out[t]["box3d_lidar"].shape[0] > 0 and bool(torch.isfinite(out[t]["box3d_lidar"]).all()) and bool(torch.isfinite(out[t]["scores"]).all()), t
    with torch.no_grad():
        x = det.reader(pts, batch_size=2)
        assert x.shape == (2, 256, 64, 64) and bool(torch.isfinite(x).all()) and bool(x.any())
        assert det.reader.pillarview.__dict__["_hip_net"]                       # the views ran on the masked HIP convolution kernels
        # an empty second frame keeps its slot: the detector hands batch_size on to the reader
        one = det({"points": pts[pts[:, 0] == 0], "token": ["a", "b"], "batch_size": 2})
        assert set(one) == {"a", "b"}


def test_mvf18_detector_training_step():
    """The gradient reaches the two view ResNets only through the sampling's backward (pnx_bilinear_gather_backward)."""
    from pillarnext_amd import config, synth

    cfg = _small_mvf18()
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().train()
    B, M = 2, 16
    H = W = 512 // cfg["_out_size_factor"][0]
    assert H == 128
    pts = torch.from_numpy(synth.make_batch("C1", B, "sweep", n=6000)).cuda()
    ex = {"points": pts, "batch_size": B, **_labels([list(t) for t in cfg["_tasks"]], B, M, H, W)}
    opt = torch.optim.SGD(det.parameters(), lr=1e-3)
    loss, _ = det(ex)
    assert bool(torch.isfinite(loss))
    opt.zero_grad()
    loss.backward()
    for view in ("pillarview", "cylinderview"):
        for k, p in getattr(det.reader, view).blocks.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), f"reader.{view}.blocks.{k}"
    opt.step()
    loss2, _ = det(ex)
    print(f"[mvf18 training step] loss {loss.item():.6f} -> {loss2.item():.6f}")
    assert bool(torch.isfinite(loss2)) and loss2.item() != loss.item()

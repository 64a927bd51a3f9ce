"""CPU: the functional view-net statement of tests/mvf_view_ref.py (the fp64 yardstick of tests/test_gpu_mvf_sparse_rows.py) is held, run in
fp32, to the modules it restates -- SingleView.blocks on the CPU, forward, running statistics and gradients -- and its active sets to the
rulebook of tests/sparse_conv3d_ref.py on a grid of depth 1."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mvf_view_ref as V  # noqa: E402
import sparse_conv3d_ref as R  # noqa: E402


def _view(layer_nums=(1, 2), strides=(1, 2), widths=(8, 12), seed=0):
    from pillarnext_amd.mvf_encoder import SingleView

    torch.manual_seed(seed)
    view = SingleView(10, [16], list(layer_nums), list(strides), list(widths), [3] * len(widths), "pillar", [0.5, 0.5, 8.0], [0.0, 0.0, -2.0, 8.0, 8.0, 4.0])
    with torch.no_grad():
        for m in view.blocks.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.3, 0.3), m.running_mean.uniform_(-0.2, 0.2), m.running_var.uniform_(0.5, 1.5)
    return view


def _cells(B, H, W, n, seed):
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(B * H * W, size=n, replace=False))
    unq = torch.from_numpy(np.stack(np.unravel_index(keys, (B, H, W)), 1)).int()
    fv = torch.from_numpy(rng.standard_normal((n, 16)).astype(np.float32))
    return unq, fv


def _modules(view, fv, unq, B, H, W):
    canvas = torch.zeros((B, H, W, fv.shape[1]))
    mask = torch.zeros((B, 1, H, W))
    u = unq.long()
    canvas = canvas.index_put((u[:, 0], u[:, 1], u[:, 2]), fv)
    mask[u[:, 0], 0, u[:, 1], u[:, 2]] = 1
    x = canvas.permute(0, 3, 1, 2)
    masks = []
    for blk in view.blocks:
        x, mask = blk(x, mask)
        masks.append(mask)
    return x, masks


@pytest.mark.parametrize("training", [True, False])
def test_twin_in_fp32_is_the_modules(training):
    B, H, W = 2, 11, 9
    view = _view().train(training)
    unq, fv = _cells(B, H, W, 60, 1)
    params, buffers = V.tensors_of(view, torch.float32)
    fv_t = fv.clone().requires_grad_(True)
    cells_xy = torch.rand((30, 2)) * torch.tensor([W / 2 + 1.0, H / 2 + 1.0]) - 0.75
    inv = torch.randint(len(unq), (30,))
    t = V.view_twin(view, fv_t, unq, cells_xy, inv, B, H, W, params, buffers)
    fv_m = fv.clone().requires_grad_(True)
    x, masks = _modules(view, fv_m, unq, B, H, W)
    scale = float(x.detach().abs().max())
    assert scale > 0.1
    assert float((t["maps"][-1] - x).detach().abs().max()) <= 2e-5 * scale
    for s, m in zip(t["sets"], masks):
        assert torch.equal(s, m[:, 0].nonzero())
    for k, v in view.blocks.named_buffers():
        if v.dtype == torch.int64:
            assert int(t["buffers"][k]) == int(v)
        else:
            assert float((t["buffers"][k] - v).abs().max()) <= 1e-5 * max(float(v.abs().max()), 1.0), k
    g = torch.randn_like(x)
    (t["maps"][-1] * g).sum().backward()
    (x * g).sum().backward()
    assert float((fv_t.grad - fv_m.grad).abs().max()) <= 1e-4 * float(fv_m.grad.abs().max())
    for k, p in view.blocks.named_parameters():
        assert float((params[k].grad - p.grad).abs().max()) <= 1e-4 * max(float(p.grad.abs().max()), 1e-6), k
    # the sampled output is bilinear_interpolate of the last map
    from pillarnext_amd.mvf_encoder import bilinear_interpolate

    b = unq.long()[inv, 0:1].float()
    assert torch.equal(t["out"], bilinear_interpolate(t["maps"][-1], torch.cat([b, cells_xy], 1)))


def test_twin_is_fp64_throughout():
    B, H, W = 2, 7, 6
    view = _view().train()
    unq, fv = _cells(B, H, W, 30, 2)
    params, buffers = V.tensors_of(view, torch.float64)
    t = V.view_twin(view, fv.double(), unq, torch.rand((5, 2), dtype=torch.float64), torch.randint(30, (5,)), B, H, W, params, buffers)
    assert t["out"].dtype == torch.float64 and all(m.dtype == torch.float64 for m in t["maps"])
    assert all(v.dtype == torch.float64 for k, v in t["buffers"].items() if not k.endswith("num_batches_tracked"))
    assert len(t["sets"]) == len(view.blocks)


@pytest.mark.parametrize("H,W", [(11, 9), (13, 25), (1, 7)])
def test_twin_sets_are_the_rulebooks_output_sets(H, W):
    """Every stage's active set = SparseConv3d's output set on a grid of depth 1 with kernel (1, 3, 3), stride (1, s, s), padding (0, 1, 1)."""
    B = 2
    view = _view(layer_nums=(0, 1, 0), strides=(1, 2, 2), widths=(4, 4, 4)).eval()
    unq, fv = _cells(B, H, W, min(20, B * H * W // 2), 3)
    params, buffers = V.tensors_of(view, torch.float64)
    t = V.view_twin(view, fv.double(), unq, torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1,), dtype=torch.int64), B, H, W, params, buffers)
    c = np.concatenate([unq.numpy()[:, :1], np.zeros((len(unq), 1), np.int64), unq.numpy()[:, 1:]], 1)
    grid = (1, H, W)
    for s, stride in zip(t["sets"], (1, 2, 2)):
        c, grid = R.output_set(c, grid, (1, 3, 3), (1, stride, stride), (0, 1, 1))
        assert np.array_equal(s.numpy(), c[:, [0, 2, 3]])
    assert tuple(t["maps"][-1].shape[2:]) == grid[1:]


def test_one_active_cell_in_training_raises_as_torch_does():
    view = _view(layer_nums=(0,), strides=(2,), widths=(4,)).train()
    params, buffers = V.tensors_of(view, torch.float64)
    unq = torch.tensor([[0, 2, 2]], dtype=torch.int32)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        V.view_twin(view, torch.ones((1, 16), dtype=torch.float64), unq, torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1,), dtype=torch.int64), 1, 5, 5,
                    params, buffers)

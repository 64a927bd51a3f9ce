"""CPU: SparseResNet3D's surface (voxel18_aspp targets, constructor, state-dict keys and both spconv weight layouts, the two voxel18 configs,
guards) and the numpy rulebook restatement of tests/sparse_conv3d_ref.py against dense fp64 F.conv3d statements on small masked grids."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import sparse_conv3d_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

VOXEL18 = dict(layer_nums=[2, 2, 2, 2], ds_layer_strides=[1, 2, 2, 2], num_input_features=5)
NUSC_CH, WAYMO_CH = [18, 36, 72, 144], [16, 32, 64, 128]


def _bn_keys(prefix, c):
    return {f"{prefix}.{k}": s for k, s in (("weight", (c,)), ("bias", (c,)), ("running_mean", (c,)), ("running_var", (c,)), ("num_batches_tracked", ()))}


def expected_state(ch, cin=5, out=128):
    keys = {}
    ins = [cin] + ch[:-1]
    for i, c in enumerate(ch):
        keys[f"blocks.{i}.0.conv.weight"] = (c, 3, 3, 3, ins[i])
        keys.update(_bn_keys(f"blocks.{i}.0.norm", c))
        for j in (1, 2):
            keys[f"blocks.{i}.{j}.block1.conv.weight"] = (c, 3, 3, 3, c)
            keys.update(_bn_keys(f"blocks.{i}.{j}.block1.norm", c))
            keys[f"blocks.{i}.{j}.conv2.weight"] = (c, 3, 3, 3, c)
            keys.update(_bn_keys(f"blocks.{i}.{j}.norm2", c))
    keys["extra_conv.0.weight"] = (ch[-1], 3, 1, 1, ch[-1])
    keys.update(_bn_keys("extra_conv.1", ch[-1]))
    keys["mapping.conv.weight"] = (out, 1, 1, 1, ch[-1])
    keys.update(_bn_keys("mapping.norm", out))
    return keys


def test_voxel18_aspp_targets_resolve():
    from pillarnext_amd import config
    from pillarnext_amd.sparse3d import SparseResNet3D

    for t in ("det3d.models.readers.voxel_encoder.VoxelFeatureNet", "det3d.models.backbones.sparse_resnet3d.SparseResNet3D",
              "det3d.models.necks.aspp.ASPPNeck", "det3d.models.heads.centerhead.CenterHead"):
        assert callable(config._locate(t)), t
    assert config._locate("det3d.models.backbones.sparse_resnet3d.SparseResNet3D") is SparseResNet3D


@pytest.mark.parametrize("ch", [NUSC_CH, WAYMO_CH])
def test_constructor_keys_and_shapes(ch):
    from pillarnext_amd import config

    m = config.instantiate({"_target_": "det3d.models.backbones.sparse_resnet3d.SparseResNet3D", "_recursive_": False, **VOXEL18,
                            "ds_num_filters": ch})
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == expected_state(ch)


def test_both_spconv_layouts_load_to_the_same_parameters():
    from pillarnext_amd.sparse3d import SparseResNet3D

    torch.manual_seed(0)
    src = SparseResNet3D(ds_num_filters=NUSC_CH, **VOXEL18)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    old = {k: (v.permute(1, 2, 3, 4, 0).contiguous() if k.endswith("weight") and v.dim() == 5 else v) for k, v in sd.items()}
    assert tuple(old["blocks.0.0.conv.weight"].shape) == (3, 3, 3, 5, 18)
    a, b = SparseResNet3D(ds_num_filters=NUSC_CH, **VOXEL18), SparseResNet3D(ds_num_filters=NUSC_CH, **VOXEL18)
    a.load_state_dict(sd)
    b.load_state_dict(old)
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(va, vb), k
        assert torch.equal(va, sd[k]), k
    with pytest.raises(RuntimeError):
        a.load_state_dict({**sd, "mapping.conv.weight": torch.zeros(128, 144)})


@pytest.mark.parametrize("name,ch,grid", [("voxel18_aspp_nusc", NUSC_CH, (1344, 1344)), ("voxel18_aspp_waymo", WAYMO_CH, (2048, 2048))])
def test_configs_instantiate_a_detector(name, ch, grid):
    from pillarnext_amd import config
    from pillarnext_amd.models import SingleStageDetector
    from pillarnext_amd.sparse3d import SparseResNet3D
    from pillarnext_amd.voxel_encoder import VoxelFeatureNet, grid_of

    cfg = config.load(os.path.join(ROOT, "configs", name + ".yaml"))
    det = config.instantiate(cfg["model"])
    assert isinstance(det, SingleStageDetector) and isinstance(det.reader, VoxelFeatureNet) and isinstance(det.backbone, SparseResNet3D)
    assert [m.num_features for m in (s[0].norm for s in det.backbone.blocks)] == ch
    r = cfg["model"]["reader"]
    assert tuple(grid_of(r["pc_range"], r["voxel_size"])) == (*grid, 40)
    assert cfg["model"]["head"]["out_size_factor"] == [4] * len(cfg["_tasks"]) and cfg["model"]["neck"]["in_channels"] == 256


def _masked_case(rng, B, grid, n, cin, zero_row=True):
    D, H, W = grid
    keys = rng.choice(B * D * H * W, size=n, replace=False)
    c = np.stack(np.unravel_index(keys, (B, D, H, W)), 1)
    c, _ = R.sort_rows(c)
    x = rng.standard_normal((n, cin))
    if zero_row:
        x[n // 2] = 0.0  # an active site whose features are all zero is still active
    return c, x


def _dense(c, x, B, grid):
    D, H, W = grid
    X = torch.zeros((B, x.shape[1], D, H, W), dtype=torch.float64)
    M = torch.zeros((B, 1, D, H, W), dtype=torch.float64)
    ci = torch.from_numpy(c)
    X[ci[:, 0], :, ci[:, 1], ci[:, 2], ci[:, 3]] = torch.from_numpy(x)
    M[ci[:, 0], 0, ci[:, 1], ci[:, 2], ci[:, 3]] = 1
    return X, M


def _rows(Y, M):
    idx = M[:, 0].nonzero()
    return idx.numpy(), Y.permute(0, 2, 3, 4, 1)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]].numpy()


def test_restatement_subm_equals_masked_dense_conv():
    rng = np.random.default_rng(1)
    B, grid = 2, (5, 6, 7)
    c, x = _masked_case(rng, B, grid, 60, 4)
    for k in (3, 1):
        w = rng.standard_normal((6, k, k, k, 4))
        got, mag = R.subm_conv3d(c, x, w, k)
        X, M = _dense(c, x, B, grid)
        Y = F.conv3d(X, torch.from_numpy(w).permute(0, 4, 1, 2, 3), padding=k // 2) * M
        oc, ref = _rows(Y, M)
        assert np.array_equal(oc, c)
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
        assert (mag >= np.abs(got) - 1e-12).all()


@pytest.mark.parametrize("kernel,stride,pad", [(3, 1, 1), (3, 2, 1), ((3, 1, 1), (2, 1, 1), 0)])
def test_restatement_sparse_conv_equals_masked_dense_conv(kernel, stride, pad):
    rng = np.random.default_rng(2)
    B, grid = 2, (7, 6, 9)
    c, x = _masked_case(rng, B, grid, 40, 3)
    k, s, p = R.triple(kernel), R.triple(stride), R.triple(pad)
    w = rng.standard_normal((5, *k, 3))
    oc, got, mag, og = R.sparse_conv3d(c, x, w, grid, k, s, p)
    X, M = _dense(c, x, B, grid)
    Mo = F.max_pool3d(M, k, s, p)
    Y = F.conv3d(X, torch.from_numpy(w).permute(0, 4, 1, 2, 3), stride=s, padding=p) * Mo
    assert tuple(Mo.shape[2:]) == og == R.out_grid(grid, k, s, p)
    rc, ref = _rows(Y, Mo)
    assert np.array_equal(oc, rc)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert (mag >= np.abs(got) - 1e-12).all()


def test_restatement_dense_view_channel_order():
    c = np.array([[0, 1, 2, 3], [1, 0, 0, 0]])
    x = np.array([[1.0, 2.0], [3.0, 4.0]])
    d = R.dense_view(c, x, 2, (2, 3, 4))
    assert d.shape == (2, 4, 3, 4)
    assert d[0, 0 * 2 + 1, 2, 3] == 1.0 and d[0, 1 * 2 + 1, 2, 3] == 2.0 and d[1, 0, 0, 0] == 3.0 and d[1, 2, 0, 0] == 4.0
    assert np.count_nonzero(d) == 4


def test_guards_raise_pnx_error():
    from pillarnext_amd._lib import PnxError
    from pillarnext_amd.sparse3d import SparseResNet3D

    m = SparseResNet3D(ds_num_filters=WAYMO_CH, **VOXEL18)
    f = torch.zeros((3, 5))
    c = torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(PnxError, match="training"):
        m.train()(f, c, [40, 64, 64])
    m.eval()
    with pytest.raises(PnxError, match="gradients"):
        m(f, c, [40, 64, 64])
    with torch.no_grad():
        with pytest.raises(PnxError, match="fp32"):
            m(f.double(), c, [40, 64, 64])
        with pytest.raises(PnxError, match="CUDA"):
            m(f, c, [40, 64, 64])

"""GPU: training of SparseResNet3D -- the gradient kernels of csrc/sparse3d.hip (pnx_sp3_transpose_map, the data gradient through pnx_sp3_conv_train,
pnx_sp3_wgrad, pnx_sp3_dense_backward) and the module's autograd path.
  - every layer kind of test_gpu_sparse3d.LAYERS against the fp64 rulebook of tests/sparse_conv3d_grad_ref.py on the operands the kernel saw:
    tmap exact; dx within 1e-6 * sum|terms| + 1e-30 (the forward's bar: the same kernel, chains no longer than the forward's); dw within
    h * 2^-24 * sum|terms| + 1e-30, h = the height of the kernel's summation tree restated from the documented split (the longest FMA chain of
    a workgroup + the partials added) -- the standard bound of fp32 accumulation in a fixed order
  - the split is reached (several partials, several K steps, a row count that is no multiple of the row tile), repeats are bit-identical
  - the whole graph on a small grid against an fp64 autograd torch statement with training-mode BatchNorm: every tensor within 2 x the error the
    same statement has in fp32 on the GPU; running statistics; eval mode with gradients
  - full size (one C2 sweep frame, and the Waymo geometry): one layer of each kind and stage from the operands its backward saw, in fp64 on the GPU
  - the detector of configs/voxel18_aspp_nusc.yaml: a training step, gradients on every backbone parameter, an SGD step that moves the loss; labels
    of another map size than the head's are refused by the fused loss."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse_conv3d_grad_ref as G  # noqa: E402
import sparse_conv3d_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_gpu_sparse3d import LAYERS, NUSC, VOXEL18, WAYMO, _case, _coords, _keys, _rel, _voxels  # noqa: E402

EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ single layers vs the fp64 rulebook
def _layer_operands(kind, kernel, stride, pad, cin, cout, res, n=500):
    from pillarnext_amd import ops

    rng = np.random.default_rng(cin * 1000 + cout + (7 if res else 0) + 100_000)
    B, grid = 2, (9, 10, 11)
    c, x = _case(rng, B, grid, n, cin)
    perm = rng.permutation(len(c))
    k, s, p = R.triple(kernel), R.triple(stride), R.triple(pad)
    w = (rng.standard_normal((cout, *k, cin)) / np.sqrt(cin * np.prod(k))).astype(np.float32)
    tc = torch.from_numpy(c[perm]).int().cuda().contiguous()
    tx = torch.from_numpy(x[perm]).cuda().contiguous()
    ix, rows, _ = ops.sp3_index_build(tc, B, grid, want_rows=True)
    if kind == "sparse":
        oix, ocnt = ops.sp3_out_index(tc, B, grid, k, s, p)
        oc = ops.sp3_index_coords(oix, int(ocnt.item()))
    else:
        oc = tc
    m = ops.sp3_neighbor_map(oc, ix, rows, k, s, p)
    ref_m = R.neighbor_map(oc.cpu().numpy(), c[perm], k, s, p)
    assert np.array_equal(m.cpu().numpy(), ref_m)
    dy = rng.standard_normal((m.shape[0], cout)).astype(np.float32)
    return x[perm], w, dy, ref_m, tx, torch.from_numpy(w).cuda(), torch.from_numpy(dy).cuda(), m


def _check_dx(dx, ref, mag, tag):
    err = np.abs(dx.cpu().numpy().astype(np.float64) - ref)
    print(f"[{tag}] dx worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms| (bar 1e-6)")
    assert (err <= 1e-6 * mag + 1e-30).all(), f"{tag}: dx worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms|"


def _check_dw(dw, ref, mag, h, tag):
    err = np.abs(dw.cpu().numpy().astype(np.float64) - ref)
    print(f"[{tag}] dw worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms| (bar h 2^-24 = {h * EPS32:.3g}, h = {h})")
    assert (err <= h * EPS32 * mag + 1e-30).all(), f"{tag}: dw worst {np.max(err / (mag + 1e-30)):.3g} of sum|terms|, bar {h * EPS32:.3g}"


@pytest.mark.parametrize("kind,kernel,stride,pad,cin,cout,res", LAYERS)
def test_layer_gradients_against_fp64_rulebook(kind, kernel, stride, pad, cin, cout, res):
    from pillarnext_amd import ops
    from pillarnext_amd.sparse3d import sparse_conv_dgrad

    x, w, dy, ref_m, tx, tw, tdy, m = _layer_operands(kind, kernel, stride, pad, cin, cout, res)
    n_in, n_out = len(x), ref_m.shape[0]
    tag = f"{kind} k{kernel} s{stride} {cin}->{cout}"
    # transposed map: exact
    tmap = ops.sp3_transpose_map(m, n_in)
    ref_t = G.transpose_map(ref_m, n_in)
    assert np.array_equal(tmap.cpu().numpy(), ref_t), "transposed map differs"
    if kind == "subm":
        assert torch.equal(tmap, m.flip(1)), "submanifold mirror identity"
    # data gradient, as the module computes it (mirrored taps on the own map for SubM, the transposed map otherwise)
    ref_dx, mag_dx = G.grad_input(ref_m, w.astype(np.float64), dy.astype(np.float64), n_in)
    dx = sparse_conv_dgrad(tdy, tw, m, n_in, subm=kind == "subm")
    assert dx.shape == (n_in, cin)
    _check_dx(dx, ref_dx, mag_dx, tag)
    if kind == "subm":  # both routes agree with the rulebook
        _check_dx(sparse_conv_dgrad(tdy, tw, m, n_in, subm=False), ref_dx, mag_dx, tag + " via tmap")
    unreached = np.setdiff1d(np.arange(n_in), ref_m[ref_m >= 0])
    assert not dx[torch.from_numpy(unreached).cuda()].any(), "dx of a row no output reaches must be exactly 0"
    assert torch.equal(dx, sparse_conv_dgrad(tdy, tw, m, n_in, subm=kind == "subm")), "dx differs between two runs"
    # weight gradient
    ref_dw, mag_dw = G.grad_weight(ref_m, x.astype(np.float64), dy.astype(np.float64))
    dw = ops.sp3_wgrad(tx, m, tdy)
    assert dw.shape == (cout, ref_m.shape[1], cin)
    _check_dw(dw, ref_dw, mag_dw, G.wgrad_tree_height(n_out, cout), tag)
    empty = torch.from_numpy(mag_dw == 0).cuda()
    assert not dw[empty].any(), "an element without a term must be exactly 0"
    assert torch.equal(dw, ops.sp3_wgrad(tx, m, tdy)), "dw differs between two runs"


# (rows, ..., what the case reaches): "split" = several partials per element, several K steps in every workgroup, a last chunk that ends inside a
# K step; "one" = a single partial whose only workgroup runs several K steps and ends inside one (fewer rows than a chunk)
@pytest.mark.parametrize("n,cin,cout,kind,kernel,stride,pad,reach", [(1500, 18, 18, "subm", 3, 1, 1, "split"), (1203, 36, 72, "subm", 3, 1, 1, "split"),
                                                                     (807, 144, 144, "subm", 1, 1, 0, "split"), (1500, 18, 36, "sparse", 3, 2, 1, "split"),
                                                                     (100, 5, 18, "subm", 3, 1, 1, "one")])
def test_wgrad_split_is_reached(n, cin, cout, kind, kernel, stride, pad, reach):
    """The launch's split, restated from include/pnx.h, really has the shape each case is there for."""
    from pillarnext_amd import ops

    x, w, dy, ref_m, tx, tw, tdy, m = _layer_operands(kind, kernel, stride, pad, cin, cout, False, n=n)
    n_out = ref_m.shape[0]
    rows, parts, mt, groups = G.wgrad_split(n_out, cout)
    print(f"n_out {n_out}: {rows} rows per workgroup, {parts} partials, {mt} channel tiles per wave in {groups} groups")
    last = n_out - (parts - 1) * rows  # rows of the last workgroup
    assert (parts > 1) == (reach == "split"), f"{parts} partials"
    assert min(rows, n_out) > 16 and last > 16, "every workgroup runs more than one K step of 16 rows"
    assert n_out % 16 != 0 and last % 16 != 0, "N_out is no multiple of the row tile: the last K step is ragged"
    assert ops.sp3_wgrad_workspace_bytes(n_out, ref_m.shape[1], cin, cout) == max(256, parts * ref_m.shape[1] * cin * cout * 4)
    ref_dw, mag_dw = G.grad_weight(ref_m, x.astype(np.float64), dy.astype(np.float64))
    dw = ops.sp3_wgrad(tx, m, tdy)
    _check_dw(dw, ref_dw, mag_dw, G.wgrad_tree_height(n_out, cout), f"split n_out {n_out} {cin}->{cout}")
    assert torch.equal(dw, ops.sp3_wgrad(tx, m, tdy))


def test_dense_gradient_is_the_gather_and_repeats():
    from pillarnext_amd import ops

    rng = np.random.default_rng(9)
    B, grid, C = 3, (2, 5, 7), 6
    c, x = _case(rng, B, grid, 90, C)
    tc = torch.from_numpy(c).int().cuda().contiguous()
    dout = torch.randn((B, C * grid[0], grid[1], grid[2]), device="cuda")
    d = ops.sp3_dense_backward(dout, tc, C)
    ref = dout.view(B, C, *grid)[tc[:, 0].long(), :, tc[:, 1].long(), tc[:, 2].long(), tc[:, 3].long()]
    assert torch.equal(d, ref) and torch.equal(d, ops.sp3_dense_backward(dout, tc, C))
    # <dense(x), dout> == <x, dense_backward(dout)>: the pair is adjoint
    tx = torch.from_numpy(x.astype(np.float32)).cuda()
    a = float((ops.sp3_dense(tx, tc, B, grid).double() * dout.double()).sum())
    b = float((tx.double() * d.double()).sum())
    assert abs(a - b) <= 1e-9 * max(abs(a), 1.0)


# ------------------------------------------------------------------------------------------------ whole graph: autograd torch statement
def _geometry(coords, grid, conv, subm):
    """Output coords, output grid and per tap (output rows, input rows) of one layer, from integer keys (torch.unique / searchsorted)."""
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    og = R.out_grid(grid, k, s, p)
    dev = coords.device
    c = coords.long()
    taps = [(a, b, d) for a in range(k[0]) for b in range(k[1]) for d in range(k[2])]
    sv, pv = torch.tensor(s, device=dev), torch.tensor(p, device=dev)
    if subm:
        oc = coords
    else:
        cand = []
        for o in taps:
            t = c[:, 1:] + pv - torch.tensor(o, device=dev)
            ok = (t >= 0).all(1) & (t % sv == 0).all(1) & (t // sv < torch.tensor(og, device=dev)).all(1)
            cand.append(_keys(torch.cat([c[ok, :1], t[ok] // sv], 1), og))
        oc = _coords(torch.unique(torch.cat(cand)), og)
    skey, order = torch.sort(_keys(coords, grid))
    q = oc.long()
    pairs = []
    for o in taps:
        pin = q[:, 1:] * sv - pv + torch.tensor(o, device=dev)
        inside = (pin >= 0).all(1) & (pin < torch.tensor(grid, device=dev)).all(1)
        key = _keys(torch.cat([q[:, :1], pin.clamp(min=0)], 1), grid)
        pos = torch.searchsorted(skey, key).clamp(max=max(len(skey) - 1, 0))
        sel = (inside & (skey[pos] == key)).nonzero()[:, 0]
        pairs.append((sel, order[pos[sel]]))
    return oc, og, pairs


def train_statement(bb, params, feats, coords, grid, B, dtype):
    """SparseResNet3D.forward in training mode as torch ops under autograd, in `dtype`: gather + matmul + index_add per tap, BatchNorm with the
    batch's own mean and biased variance (eps 1e-3).  -> (active sets, dense output, {norm name: (batch mean, biased batch variance, rows)})."""
    stats = {}

    def conv(x, name, coords, grid, mod, subm):
        oc, og, pairs = _geometry(coords, grid, mod, subm)
        w = params[name + ".weight"]
        out = torch.zeros((oc.shape[0], w.shape[0]), dtype=dtype, device=x.device)
        k = mod.kernel_size
        for ti, (sel, src) in enumerate(pairs):
            o = (ti // (k[1] * k[2]), (ti // k[2]) % k[1], ti % k[2])
            out = out.index_add(0, sel, x[src] @ w[:, o[0], o[1], o[2], :].T)
        return oc, out, og

    def bn(x, name):
        mean, var = x.mean(0), x.var(0, unbiased=False)
        stats[name] = (mean.detach(), var.detach(), x.shape[0])
        return (x - mean) / torch.sqrt(var + 1e-3) * params[name + ".weight"] + params[name + ".bias"]

    x = feats.to(dtype)
    sets = []
    for i, seq in enumerate(bb.blocks):
        coords, x, grid = conv(x, f"blocks.{i}.0.conv", coords, grid, seq[0].conv, False)
        x = torch.relu(bn(x, f"blocks.{i}.0.norm"))
        for j, blk in enumerate(seq[1:], 1):
            y = torch.relu(bn(conv(x, f"blocks.{i}.{j}.block1.conv", coords, grid, blk.block1.conv, True)[1], f"blocks.{i}.{j}.block1.norm"))
            x = torch.relu(bn(conv(y, f"blocks.{i}.{j}.conv2", coords, grid, blk.conv2, True)[1], f"blocks.{i}.{j}.norm2") + x)
        sets.append((coords, x))
    coords, x, grid = conv(x, "extra_conv.0", coords, grid, bb.extra_conv[0], False)
    x = torch.relu(bn(x, "extra_conv.1"))
    sets.append((coords, x))
    x = torch.relu(bn(conv(x, "mapping.conv", coords, grid, bb.mapping.conv, True)[1], "mapping.norm"))
    sets.append((coords, x))
    D, H, W = grid
    c = coords.long()
    dense = torch.zeros((B, D, H, W, x.shape[1]), dtype=dtype, device=x.device).index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), x)
    return sets, dense.permute(0, 4, 1, 2, 3).reshape(B, -1, H, W), stats


def _train_backbone(ch, seed):
    from pillarnext_amd.sparse3d import SparseResNet3D

    torch.manual_seed(seed)
    bb = SparseResNet3D(ds_num_filters=ch, **VOXEL18)
    with torch.no_grad():
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.2, 0.2), m.running_mean.uniform_(-0.2, 0.2), m.running_var.uniform_(0.5, 2.0)
    return bb.cuda().train()


def _small_scene():
    grid = (40, 20, 24)
    D, H, W = grid
    rng = np.random.default_rng(5)
    faces = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(0, 7, 9), (D - 1, 3, 4), (5, 0, 11), (6, H - 1, 2), (4, 8, 0),
                                                                                      (7, 13, W - 1)]
    inner = [tuple(v) for v in np.stack(np.unravel_index(rng.choice(D * H * W, 150, replace=False), grid), 1)]
    rows = sorted({(b, *v) for b in (0, 2) for v in faces + inner})  # sample 1 of 3 is empty
    coords = torch.tensor(rows, dtype=torch.int32, device="cuda")
    torch.manual_seed(11)
    return torch.randn((len(rows), 5), device="cuda"), coords, grid


def test_whole_graph_against_fp64_autograd_statement():
    """ratio = the HIP module's relative Frobenius error / the fp32 torch statement's, both against the fp64 statement; bar 2 per tensor (the
    measured ratios are in CHANGELOG.md)."""
    bb = _train_backbone([16, 32, 64, 128], seed=3)
    feats, coords, grid = _small_scene()
    B = 3
    start = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    proj = torch.randn((B, 256, 3, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

    def statement(dtype):
        params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in bb.named_parameters()}
        f = feats.detach().to(dtype).clone().requires_grad_(True)
        sets, dense, stats = train_statement(bb, params, f, coords, grid, B, dtype)
        (dense * proj.to(dtype)).sum().backward()
        return sets, dense.detach(), {**{k: p.grad for k, p in params.items()}, "input features": f.grad}, stats

    sets64, out64, g64, stats = statement(torch.float64)
    sets32, out32, g32, _ = statement(torch.float32)
    f = feats.detach().clone().requires_grad_(True)
    sets = bb.forward_sparse(f, coords, grid, B)
    assert len(sets) == len(sets64) == 6
    for i, ((c, x, _), (rc, rx)) in enumerate(zip(sets, sets64)):
        assert torch.equal(c, rc), f"active set {i} differs"
    bb.load_state_dict(start)  # forward_sparse above moved the running statistics once
    out = bb(f, coords, grid, B)
    assert out.shape == out64.shape == (3, 256, 3, 3) and not bool(out[1].any())
    (out * proj).sum().backward()
    got = {**{k: p.grad for k, p in bb.named_parameters()}, "input features": f.grad}
    worst = 0.0
    rows = [("dense output", _rel(out.detach(), out64), _rel(out32, out64))]
    for k, r in g64.items():
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), k
        rows.append((k, _rel(got[k], r), _rel(g32[k], r)))
    for k, e_hip, e_32 in rows:
        print(f"[whole graph] {k:34s} HIP {e_hip:.3g}  fp32 torch {e_32:.3g}  ratio {e_hip / max(e_32, 1e-300):.2f}")
        worst = max(worst, e_hip / max(e_32, 1e-300))
    print(f"[whole graph] worst ratio {worst:.2f} (bar 2)")
    for k, e_hip, e_32 in rows:
        assert e_hip <= 2 * e_32, f"{k}: HIP {e_hip:.3g} vs fp32 torch statement {e_32:.3g}"
    # running statistics as nn.BatchNorm1d keeps them: momentum 0.01, unbiased variance
    for name, (mean, var, n) in stats.items():
        bn = bb.get_submodule(name)
        assert int(bn.num_batches_tracked) == int(start[name + ".num_batches_tracked"]) + 1
        want_m = 0.99 * start[name + ".running_mean"].double() + 0.01 * mean
        want_v = 0.99 * start[name + ".running_var"].double() + 0.01 * var * n / (n - 1)
        assert _rel(bn.running_mean, want_m) <= 1e-5 and _rel(bn.running_var, want_v) <= 1e-5, name


def test_eval_mode_with_gradients_and_repeats():
    bb = _train_backbone([16, 32, 64, 128], seed=4).eval()
    feats, coords, grid = _small_scene()
    before = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    with torch.no_grad():
        folded = bb(feats, coords, grid, 3)
    out = bb(feats, coords, grid, 3)  # gradients enabled, parameters require them: the autograd path on the running statistics
    assert out.requires_grad and _rel(out.detach(), folded.double()) <= 1e-5
    out.sum().backward()
    for k, p in bb.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    for k, v in bb.state_dict().items():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"
    first = {k: p.grad.clone() for k, p in bb.named_parameters()}
    bb.zero_grad(set_to_none=True)
    f = feats.clone().requires_grad_(True)
    bb(f, coords, grid, 3).sum().backward()
    for k, p in bb.named_parameters():
        assert torch.equal(p.grad, first[k]), f"{k}: gradient differs between two runs"
    assert f.grad is not None and bool(torch.isfinite(f.grad).all()) and bool(f.grad.any())
    for p in bb.parameters():
        p.requires_grad_(False)
    assert not bb(feats, coords, grid, 3).requires_grad  # nothing wants a gradient: the folded path
    assert torch.equal(bb(feats, coords, grid, 3), folded)


# ------------------------------------------------------------------------------------------------ full size, layer by layer
def _fp64_layer_grads(x, m, dy, w):
    """dx, dw and the sum of |terms| of each, tap by tap in fp64 on the GPU."""
    co, ci = w.shape[0], w.shape[-1]
    T = m.shape[1]
    wt = w.double().reshape(co, T, ci)
    x64, dy64 = x.double(), dy.double()
    dx, dxm = torch.zeros_like(x64), torch.zeros_like(x64)
    dw, dwm = torch.zeros((co, T, ci), dtype=torch.float64, device=x.device), torch.zeros((co, T, ci), dtype=torch.float64, device=x.device)
    for t in range(T):
        o = (m[:, t] >= 0).nonzero()[:, 0]
        src = m[o, t].long()
        g = dy64[o]
        dx.index_add_(0, src, g @ wt[:, t])  # at most one output row per input row and tap: no two terms of a tap meet
        dxm.index_add_(0, src, g.abs() @ wt[:, t].abs())
        xs = x64[src]
        dw[:, t] = g.T @ xs
        dwm[:, t] = g.abs().T @ xs.abs()
    return dx, dxm, dw, dwm


@pytest.mark.parametrize("name,config,geom,ch", [("nusc", "C2", NUSC, [18, 36, 72, 144]), ("waymo", "C5ref", WAYMO, [16, 32, 64, 128])])
def test_full_size_layer_gradients(name, config, geom, ch, monkeypatch):
    from pillarnext_amd import ops, sparse3d

    feats, coords, grid = _voxels(config, geom, 1)
    bb = _train_backbone(ch, seed=0)
    seen = {}
    real = sparse3d.SparseConvFunction

    class Recording:
        @staticmethod
        def apply(x, weight, nbmap, subm, tick):
            y = real.apply(x, weight, nbmap, subm, tick)
            rec = {"x": x.detach(), "map": nbmap, "subm": subm, "weight": weight}
            y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().contiguous().clone()))
            seen[len(seen)] = rec
            return y

    monkeypatch.setattr(sparse3d, "SparseConvFunction", Recording)
    f = feats.detach().clone().requires_grad_(True)
    out = bb(f, coords, grid, 1)
    proj = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    (out * proj).sum().backward()
    monkeypatch.undo()
    order = [n for i, seq in enumerate(bb.blocks) for n in [f"blocks.{i}.0.conv"] + [f"blocks.{i}.{j}.{c}" for j in (1, 2) for c in ("block1.conv", "conv2")]]
    order += ["extra_conv.0", "mapping.conv"]
    assert len(seen) == len(order) == 22
    recs = dict(zip(order, seen.values()))
    picked = [f"blocks.{i}.0.conv" for i in range(4)] + [f"blocks.{i}.1.conv2" for i in range(4)] + ["extra_conv.0", "mapping.conv"]
    for lname in picked:
        r = recs[lname]
        assert r["weight"] is bb.get_submodule(lname).weight
        w = r["weight"].detach()
        x, m, dy = r["x"], r["map"], r["dy"]
        n_out, cout = dy.shape
        dx64, dxm, dw64, dwm = _fp64_layer_grads(x, m, dy, w)
        dx = sparse3d.sparse_conv_dgrad(dy, w, m, x.shape[0], r["subm"])
        err = (dx.double() - dx64).abs()
        wdx = float((err / (dxm + 1e-30)).max())
        dw = ops.sp3_wgrad(x, m, dy)
        h = G.wgrad_tree_height(n_out, cout)
        errw = (dw.double() - dw64).abs()
        wdw = float((errw / (dwm + 1e-30)).max())
        rows, parts, _, _ = G.wgrad_split(n_out, cout)
        print(f"[{name}] {lname:22s} {x.shape[0]:8d} -> {n_out:8d} rows, {x.shape[1]:3d} -> {cout:3d}: dx worst {wdx:.3g} (bar 1e-6), "
              f"dw worst {wdw:.3g} (bar {h * EPS32:.3g}: {rows} rows per workgroup + {parts} partials)")
        assert bool((err <= 1e-6 * dxm + 1e-30).all()), f"{lname}: dx worst {wdx:.3g} of sum|terms|"
        assert bool((errw <= h * EPS32 * dwm + 1e-30).all()), f"{lname}: dw worst {wdw:.3g} of sum|terms|, bar {h * EPS32:.3g}"
        # the module's own gradient is this kernel's output: every weight is used once
        assert torch.equal(bb.get_submodule(lname).weight.grad, dw.view(w.shape)), lname
    assert f.grad is not None and bool(torch.isfinite(f.grad).all())


# ------------------------------------------------------------------------------------------------ detector: a training step
def _labels(tasks, B, M, H, W, seed=3):
    """Random targets as tests/test_gpu_decode.py and tools/train_step.py build them for the pillar detector."""
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


def test_fused_loss_refuses_labels_of_another_map_size():
    """The kernels read the targets through raw pointers with the head map's extents: a target of another size must raise, not be read past its end."""
    from pillarnext_amd._lib import PnxError
    from pillarnext_amd.losses import fused_center_loss

    B, M = 2, 8
    pd = {k: torch.zeros((B, c, 24, 24), device="cuda") for k, c in (("hm", 2), ("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("iou", 1))}
    ex = _labels([["a", "b"]], B, M, 12, 12)
    args = (ex["ind"][0], ex["mask"][0], ex["cat"][0], ex["anno_box"][0], ex["gt_boxes"][0], (0.3, 0.3, -50.4, -50.4), True)
    with pytest.raises(PnxError, match="hm target"):
        fused_center_loss(pd, ex["hm"][0], *args)
    with pytest.raises(PnxError, match="head map"):
        fused_center_loss({**pd, "dim": pd["dim"][:, :, :12, :12]}, _labels([["a", "b"]], B, M, 24, 24)["hm"][0], *args)


def test_voxel18_nusc_detector_training_step():
    """The head's maps are grid / out_size_factor = 1344 / 4 = 336 cells wide (the 168-wide backbone output through the stride-2 deblock)."""
    from pillarnext_amd import config, synth

    cfg = config.load(os.path.join(ROOT, "configs", "voxel18_aspp_nusc.yaml"))
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().train()
    B, M = 2, 16
    H = W = 1344 // cfg["_out_size_factor"][0]
    assert H == 336
    pts = torch.from_numpy(synth.make_batch("C2ref", B, "sweep", n=60_000)).cuda()
    ex = {"points": pts, "batch_size": B, **_labels([list(t) for t in cfg["_tasks"]], B, M, H, W)}
    opt = torch.optim.SGD(det.parameters(), lr=1e-3)
    loss, _ = det(ex)
    assert bool(torch.isfinite(loss))
    opt.zero_grad()
    loss.backward()
    for k, p in det.backbone.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), f"backbone.{k}"
    opt.step()
    loss2, _ = det(ex)
    print(f"[voxel18 training step] loss {float(loss):.6f} -> {float(loss2):.6f}")
    assert bool(torch.isfinite(loss2)) and float(loss2) != float(loss)

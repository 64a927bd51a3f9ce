"""GPU: SparseResNet3D's 16-bit training path -- pnx_sp3_conv_h_f32 (forward and data gradient), pnx_sp3_wgrad_h and SparseConvHalfFunction,
in bf16 and fp16, against the fp64 statement of tests/sparse3d_half_train_ref.py ON THE OPERANDS THE KERNELS SAW (ops.sp3_rows_h and
ops.sp3_pack_weight_h are asserted to give round_to's bits first).
  - the default did not change: SparseConvFunction and the fp32 module give the same bits before, while and after the option is on elsewhere
  - every layer of test_gpu_sparse3d.LAYERS: y and dx within 1e-6 * sum|terms| + 1e-30, dw within h * 2^-24 * sum|terms| + 1e-30 (h = terms of
    the longest chain of the documented split + partials added), exact zeros where there is no term, bit-identical repeats
  - the weight gradient's split is reached: several partials, a last workgroup that ends inside a K step of 32, fewer than 32 rows, a multiple
    of 32, narrow / ragged channel tiles at T = 1, a stride-2 layer, a tap no row has
  - SubM data gradient: mirrored taps on the own map and the transposed map BOTH meet the layer bar (they sum the taps in opposite order, so
    their bits may differ)
  - the whole small backbone in training mode: (a) fp64 autograd, (b) fp64 with the rounding node, (c) the module; |c - a| <= 1.5 |b - a| for
    the output, 2 |b - a| for every gradient; running statistics, eval mode with gradients, a second backward
  - the voxel18 detector: one training step with the option on."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse3d_half_ref as HR  # noqa: E402
import sparse3d_half_train_ref as TR  # noqa: E402
from conftest import ROOT  # noqa: E402
from sparse3d_half_ref import round_to  # noqa: E402
from test_gpu_sparse3d import LAYERS  # noqa: E402
from test_gpu_sparse3d_grad import _geometry, _labels, _layer_operands, _small_scene, _train_backbone  # noqa: E402

EPS32 = 2.0 ** -24
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def _rows(t, c, dtype, ref64):
    """ops.sp3_rows_h(t) -- asserted to hold exactly round_to(ref64) in its first c columns and zeros in the pad columns."""
    from pillarnext_amd import ops

    h = ops.sp3_rows_h(t, dtype)
    assert h.dtype == dtype and tuple(h.shape) == (t.shape[0], (c + 7) // 8 * 8) and h.is_contiguous()
    assert np.array_equal(h[:, :c].double().cpu().numpy(), round_to(ref64, dtype)) and not bool(h[:, c:].any())
    return h


def _worst(got, ref, mag):
    err = np.abs(got.double().cpu().numpy() - ref)
    return err, float(np.max(err / (mag + 1e-30))) if err.size else 0.0


# ------------------------------------------------------------------------------------------------ 6. the default did not change
def test_default_paths_are_unchanged_by_the_option():
    """First in the file: the fp32 node and the fp32 module before any module of this process has the option on, then again while another module
    runs with it and after this one had it switched on and off."""
    from pillarnext_amd import ops
    from pillarnext_amd.sparse3d import SparseConvFunction

    x, w, dy, ref_m, tx, tw, tdy, m = _layer_operands("subm", 3, 1, 1, 18, 18, False)

    def node():
        a, b = tx.clone().requires_grad_(True), tw.clone().requires_grad_(True)
        y = SparseConvFunction.apply(a, b, m, True, lambda phase: None)
        y.backward(tdy)
        return y.detach(), a.grad, b.grad

    def module(bb):
        bb.zero_grad(set_to_none=True)
        f = feats.clone().requires_grad_(True)
        out = bb(f, coords, grid, 3)
        out.sum().backward()
        return [out.detach(), f.grad] + [p.grad.clone() for p in bb.parameters()]

    feats, coords, grid = _small_scene()
    bb = _train_backbone([16, 32, 64, 128], seed=6).eval()  # eval mode with gradients: the autograd path on fixed statistics
    before_node, before_mod = node(), module(bb)
    other = _train_backbone([16, 32, 64, 128], seed=6).eval().use_half_precision(torch.bfloat16, training=True)
    half = module(other)
    assert not torch.equal(half[0], before_mod[0]), "the option changes nothing: the 16-bit node is not reached"
    for a, b in zip(node(), before_node):
        assert torch.equal(a, b), "SparseConvFunction changed while the option is on in another module"
    bb.use_half_precision(torch.float16, training=True)
    module(bb)
    bb.use_half_precision(None)
    for a, b in zip(module(bb), before_mod):
        assert torch.equal(a, b), "the fp32 autograd path changed after the option was switched on and off"
    bb.use_half_precision(torch.bfloat16)  # training=False: inference only, as before
    for a, b in zip(module(bb), before_mod):
        assert torch.equal(a, b), "use_half_precision(dtype) without training=True touched the autograd path"
    for a, b in zip(node(), before_node):
        assert torch.equal(a, b)
    assert ops.sp3_wgrad(tx, m, tdy).shape == (18, 27, 18)


# ------------------------------------------------------------------------------------------------ 1. single layers vs the fp64 statement
def _layer_half(kind, kernel, stride, pad, cin, cout, dtype, n=500):
    from pillarnext_amd import ops

    x, w, dy, ref_m, tx, tw, tdy, m = _layer_operands(kind, kernel, stride, pad, cin, cout, False, n=n)
    xh, dyh = _rows(tx, cin, dtype, x.astype(np.float64)), _rows(tdy, cout, dtype, dy.astype(np.float64))
    wp = ops.sp3_pack_weight_h(tw, dtype)
    assert np.array_equal(wp.double().cpu().numpy(), HR.pack_weight_h_ref(w, dtype)), "packed weights are not round_to(w) in fragment order"
    return x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), ref_m, xh, tw, dyh, wp, m


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,kernel,stride,pad,cin,cout,res", LAYERS)
def test_layer_against_fp64_statement(kind, kernel, stride, pad, cin, cout, res, dtype):
    from pillarnext_amd import ops
    from pillarnext_amd.sparse3d import sparse_conv_dgrad_h

    x, w, dy, ref_m, xh, tw, dyh, wp, m = _layer_half(kind, kernel, stride, pad, cin, cout, dtype)
    n_in, n_out, subm = len(x), ref_m.shape[0], kind == "subm"
    tag = f"{IDS[DTYPES.index(dtype)]} {kind} k{kernel} s{stride} {cin}->{cout}"
    # forward
    y = ops.sp3_conv_h_f32(xh, m, wp, cin, cout)
    assert y.dtype == torch.float32 and tuple(y.shape) == (n_out, cout)
    ref_y, mag_y = TR.forward(ref_m, x, w, dtype)
    err, worst_y = _worst(y, ref_y, mag_y)
    assert (err <= 1e-6 * mag_y + 1e-30).all(), f"{tag}: y worst {worst_y:.3g} of sum|terms|"
    assert not y[torch.from_numpy(mag_y.sum(1) == 0).cuda()].any(), "y of a row without a neighbour must be exactly 0"
    assert torch.equal(y, ops.sp3_conv_h_f32(xh, m, wp, cin, cout)), "y differs between two runs"
    # data gradient, as the node computes it
    dx = sparse_conv_dgrad_h(dyh, tw, m, n_in, subm)
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (n_in, cin)
    ref_dx, mag_dx = TR.grad_input(ref_m, w, dy, n_in, dtype)
    err, worst_dx = _worst(dx, ref_dx, mag_dx)
    assert (err <= 1e-6 * mag_dx + 1e-30).all(), f"{tag}: dx worst {worst_dx:.3g} of sum|terms|"
    unreached = np.setdiff1d(np.arange(n_in), ref_m[ref_m >= 0])
    assert not dx[torch.from_numpy(unreached).cuda()].any(), "dx of a row no output reaches must be exactly 0"
    assert torch.equal(dx, sparse_conv_dgrad_h(dyh, tw, m, n_in, subm)), "dx differs between two runs"
    # weight gradient
    dw = ops.sp3_wgrad_h(xh, m, dyh, cin, cout)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (cout, ref_m.shape[1], cin)
    ref_dw, mag_dw = TR.grad_weight(ref_m, x, dy, dtype)
    h = TR.wgrad_h_tree_height(n_out, cout)
    err, worst_dw = _worst(dw, ref_dw, mag_dw)
    print(f"[{tag}] worst of sum|terms|: y {worst_y:.3g}, dx {worst_dx:.3g} (bar 1e-6), dw {worst_dw:.3g} (bar h 2^-24 = {h * EPS32:.3g}, h = {h})")
    assert (err <= h * EPS32 * mag_dw + 1e-30).all(), f"{tag}: dw worst {worst_dw:.3g} of sum|terms|, bar {h * EPS32:.3g}"
    assert not dw[torch.from_numpy(mag_dw == 0).cuda()].any(), "an element without a term must be exactly 0"
    assert torch.equal(dw, ops.sp3_wgrad_h(xh, m, dyh, cin, cout)), "dw differs between two runs"


# ------------------------------------------------------------------------------------------------ 2. the weight gradient's split
# reach: "split" several partials, the last workgroup ends inside a K step; "even" several partials, n_out a multiple of 32; "one" a single
# partial of several K steps that ends inside one; "tiny" fewer than 32 rows, one ragged K step
SPLIT_CASES = [(1500, 18, 18, "subm", 3, 1, 1, "split"), (1203, 36, 72, "subm", 3, 1, 1, "split"), (1500, 18, 36, "sparse", 3, 2, 1, "sparse"),
               (807, 144, 144, "subm", 1, 1, 0, "split"), (1203, 36, 72, "subm", 1, 1, 0, "split"), (1500, 18, 18, "subm", 1, 1, 0, "split"),
               (100, 5, 18, "subm", 1, 1, 0, "one"), (20, 18, 18, "subm", 3, 1, 1, "tiny"), (1024, 5, 18, "subm", 3, 1, 1, "even")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,cin,cout,kind,kernel,stride,pad,reach", SPLIT_CASES)
def test_wgrad_h_split_is_reached(n, cin, cout, kind, kernel, stride, pad, reach, dtype):
    """The launch's split, restated from include/pnx.h, really has the shape each case is there for."""
    from pillarnext_amd import ops

    x, w, dy, ref_m, xh, tw, dyh, wp, m = _layer_half(kind, kernel, stride, pad, cin, cout, dtype, n=n)
    n_out, T = ref_m.shape
    rows, parts, mt, groups = TR.wgrad_h_split(n_out, cout)
    last = n_out - (parts - 1) * rows  # rows of the last workgroup
    print(f"n_out {n_out}: {rows} rows per workgroup, {parts} partials (last {last} rows), {mt} channel tiles per wave in {groups} groups")
    if reach == "split":
        assert parts > 1 and last > 32 and last % 32 != 0
    elif reach == "sparse":
        assert parts > 1 and stride == 2 and n_out != n
    elif reach == "even":
        assert parts > 1 and n_out % 32 == 0 and last % 32 == 0
    elif reach == "one":
        assert parts == 1 and n_out > 32 and n_out % 32 != 0
    else:
        assert parts == 1 and n_out < 32
    assert ops.sp3_wgrad_h_partials_bytes(n_out, T, cin, cout) == TR.wgrad_h_partials_bytes(n_out, T, cin, cout)
    ref_dw, mag_dw = TR.grad_weight(ref_m, x, dy, dtype)
    dw = ops.sp3_wgrad_h(xh, m, dyh, cin, cout)
    h = TR.wgrad_h_tree_height(n_out, cout)
    err, worst = _worst(dw, ref_dw, mag_dw)
    print(f"[split n_out {n_out} {cin}->{cout} T {T}] dw worst {worst:.3g} of sum|terms| (bar {h * EPS32:.3g}, h = {h})")
    assert (err <= h * EPS32 * mag_dw + 1e-30).all(), f"dw worst {worst:.3g} of sum|terms|, bar {h * EPS32:.3g}"
    assert not dw[torch.from_numpy(mag_dw == 0).cuda()].any()
    assert torch.equal(dw, ops.sp3_wgrad_h(xh, m, dyh, cin, cout))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wgrad_h_tap_that_no_row_has(dtype):
    from pillarnext_amd import ops

    x, w, dy, ref_m, xh, tw, dyh, wp, m = _layer_half("subm", 3, 1, 1, 18, 18, dtype, n=700)
    ref_m, m = ref_m.copy(), m.clone()
    ref_m[:, 5], ref_m[:, 26] = -1, -1
    m[:, 5], m[:, 26] = -1, -1
    m[3, 7] = len(x)  # an entry past the last input row contributes nothing either
    ref_m[3, 7] = -1
    assert TR.wgrad_h_split(700, 18)[1] > 1
    ref_dw, mag_dw = TR.grad_weight(ref_m, x, dy, dtype)
    dw = ops.sp3_wgrad_h(xh, m, dyh, 18, 18)
    assert not dw[:, 5].any() and not dw[:, 26].any() and bool(dw[:, 4].any()), "the slice of a tap no row has must be exactly 0"
    err, worst = _worst(dw, ref_dw, mag_dw)
    assert (err <= TR.wgrad_h_tree_height(700, 18) * EPS32 * mag_dw + 1e-30).all(), f"dw worst {worst:.3g}"


def test_wgrad_h_without_rows_is_zero():
    from pillarnext_amd import ops

    x = torch.zeros((0, 8), dtype=torch.bfloat16, device="cuda")
    dw = ops.sp3_wgrad_h(x, torch.zeros((0, 27), dtype=torch.int32, device="cuda"), torch.zeros((0, 24), dtype=torch.bfloat16, device="cuda"), 5, 18)
    assert tuple(dw.shape) == (18, 27, 5) and not dw.any()


# ------------------------------------------------------------------------------------------------ 3. the two dgrad routes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kernel,pad,cin,cout", [(k, p, ci, co) for kind, k, s, p, ci, co, res in LAYERS if kind == "subm" and not res])
def test_subm_dgrad_routes_both_meet_the_bar(kernel, pad, cin, cout, dtype):
    """Mirrored taps on the own map walk K = (tap, channel) with the taps reversed relative to the transposed map: the same terms in another
    order, so the bits may differ; each route is held to the layer bar on its own."""
    from pillarnext_amd.sparse3d import sparse_conv_dgrad_h

    x, w, dy, ref_m, xh, tw, dyh, wp, m = _layer_half("subm", kernel, 1, pad, cin, cout, dtype)
    ref_dx, mag_dx = TR.grad_input(ref_m, w, dy, len(x), dtype)
    for subm in (True, False):
        dx = sparse_conv_dgrad_h(dyh, tw, m, len(x), subm)
        err, worst = _worst(dx, ref_dx, mag_dx)
        print(f"[subm dgrad {cin}->{cout} k{kernel}] {'mirrored taps, own map' if subm else 'transposed map'}: worst {worst:.3g} of sum|terms|")
        assert (err <= 1e-6 * mag_dx + 1e-30).all(), f"subm={subm}: dx worst {worst:.3g} of sum|terms|"


# ------------------------------------------------------------------------------------------------ 4. the whole graph
def _statement(bb, params, feats, coords, grid, B, dtype):
    """SparseResNet3D.forward in training mode in fp64 under autograd, every convolution through TR.RoundedConv (dtype None: no rounding)."""
    def conv(x, name, coords, grid, mod, subm):
        oc, og, pairs = _geometry(coords, grid, mod, subm)
        return oc, TR.RoundedConv.apply(x, params[name + ".weight"], pairs, oc.shape[0], dtype), og

    def bn(x, name):
        mean, var = x.mean(0), x.var(0, unbiased=False)
        return (x - mean) / torch.sqrt(var + 1e-3) * params[name + ".weight"] + params[name + ".bias"]

    x = feats
    for i, seq in enumerate(bb.blocks):
        coords, x, grid = conv(x, f"blocks.{i}.0.conv", coords, grid, seq[0].conv, False)
        x = torch.relu(bn(x, f"blocks.{i}.0.norm"))
        for j, blk in enumerate(seq[1:], 1):
            y = torch.relu(bn(conv(x, f"blocks.{i}.{j}.block1.conv", coords, grid, blk.block1.conv, True)[1], f"blocks.{i}.{j}.block1.norm"))
            x = torch.relu(bn(conv(y, f"blocks.{i}.{j}.conv2", coords, grid, blk.conv2, True)[1], f"blocks.{i}.{j}.norm2") + x)
    coords, x, grid = conv(x, "extra_conv.0", coords, grid, bb.extra_conv[0], False)
    x = torch.relu(bn(x, "extra_conv.1"))
    x = torch.relu(bn(conv(x, "mapping.conv", coords, grid, bb.mapping.conv, True)[1], "mapping.norm"))
    D, H, W = grid
    c = coords.long()
    dense = torch.zeros((B, D, H, W, x.shape[1]), dtype=x.dtype, device=x.device).index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), x)
    return dense.permute(0, 4, 1, 2, 3).reshape(B, -1, H, W)


def _norm(t):
    return float(torch.linalg.vector_norm(t.double()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_whole_graph_against_fp64_statements(dtype):
    """(a) fp64 autograd, (b) fp64 autograd with the rounding node at every convolution, (c) the module with the option on.
    |c - a| <= 1.5 |b - a| for the dense output, 2 |b - a| for dL/dx and every parameter gradient."""
    bb = _train_backbone([16, 32, 64, 128], seed=3).use_half_precision(dtype, training=True)
    feats, coords, grid = _small_scene()
    B = 3
    start = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    proj = torch.randn((B, 256, 3, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

    def statement(rounding):
        params = {k: v.detach().double().clone().requires_grad_(True) for k, v in bb.named_parameters()}
        f = feats.detach().double().clone().requires_grad_(True)
        dense = _statement(bb, params, f, coords, grid, B, rounding)
        (dense * proj.double()).sum().backward()
        return dense.detach(), {**{k: p.grad for k, p in params.items()}, "input features": f.grad}

    out_a, g_a = statement(None)
    out_b, g_b = statement(dtype)
    f = feats.detach().clone().requires_grad_(True)
    out = bb(f, coords, grid, B)
    assert out.dtype == torch.float32 and out.shape == out_a.shape
    (out * proj).sum().backward()
    got = {**{k: p.grad for k, p in bb.named_parameters()}, "input features": f.grad}
    rows = [("dense output", _norm(out.detach().double() - out_a), _norm(out_b - out_a), 1.5)]
    for k, r in g_a.items():
        assert got[k] is not None and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        rows.append((k, _norm(got[k].double() - r), _norm(g_b[k] - r), 2.0))
    worst = {1.5: 0.0, 2.0: 0.0}
    for k, e_c, e_b, bar in rows:
        print(f"[whole graph {dtype}] {k:34s} |c - a| {e_c:.3g}  |b - a| {e_b:.3g}  ratio {e_c / max(e_b, 1e-300):.3f} (bar {bar})")
        worst[bar] = max(worst[bar], e_c / max(e_b, 1e-300))
    print(f"[whole graph {dtype}] worst ratio: output {worst[1.5]:.3f} (bar 1.5), gradients {worst[2.0]:.3f} (bar 2)")
    for k, e_c, e_b, bar in rows:
        assert e_c <= bar * e_b, f"{k}: |c - a| {e_c:.3g} > {bar} x |b - a| {e_b:.3g}"
    # running statistics moved, once
    for name, m in bb.named_modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            assert int(m.num_batches_tracked) == int(start[name + ".num_batches_tracked"]) + 1
            assert not torch.equal(m.running_mean, start[name + ".running_mean"]) and not torch.equal(m.running_var, start[name + ".running_var"]), name
    # a second backward from the same start gives the same bits
    first = {k: v.clone() for k, v in got.items()}
    bb.load_state_dict(start)
    bb.zero_grad(set_to_none=True)
    f2 = feats.detach().clone().requires_grad_(True)
    out2 = bb(f2, coords, grid, B)
    # the first forward ran from `start` as well: same statistics, same bits
    (out2 * proj).sum().backward()
    again = {**{k: p.grad for k, p in bb.named_parameters()}, "input features": f2.grad}
    for k in first:
        assert torch.equal(first[k], again[k]), f"{k}: gradient differs between two runs"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eval_mode_with_gradients_takes_the_same_node(dtype, monkeypatch):
    from pillarnext_amd import sparse3d

    bb = _train_backbone([16, 32, 64, 128], seed=4).eval().use_half_precision(dtype, training=True)
    feats, coords, grid = _small_scene()
    before = {k: v.detach().clone() for k, v in bb.state_dict().items()}
    calls = []
    real = sparse3d.SparseConvHalfFunction

    class Counting:
        @staticmethod
        def apply(*args):
            calls.append(args[5])
            return real.apply(*args)

    monkeypatch.setattr(sparse3d, "SparseConvHalfFunction", Counting)

    class Refusing:
        @staticmethod
        def apply(*args):
            pytest.fail("the fp32 node ran with the option on")

    monkeypatch.setattr(sparse3d, "SparseConvFunction", Refusing)
    out = bb(feats, coords, grid, 3)  # gradients enabled, parameters require them
    monkeypatch.undo()
    assert calls == [dtype] * 22 and out.requires_grad and out.dtype == torch.float32
    sets = bb.forward_sparse(feats, coords, grid, 3)
    assert all(x.dtype == torch.float32 for _, x, _ in sets)  # fp32 features on the autograd path
    out.sum().backward()
    for k, p in bb.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    for k, v in bb.state_dict().items():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"
    with torch.no_grad():
        folded = bb(feats, coords, grid, 3)  # no gradient wanted: the folded 16-bit inference path, as before
    assert not folded.requires_grad and float((folded - out.detach()).abs().max()) <= 0.1 * float(out.detach().abs().max())


# ------------------------------------------------------------------------------------------------ 5. detector: a training step
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_voxel18_nusc_detector_training_step_half(dtype):
    from pillarnext_amd import config, synth

    cfg = config.load(os.path.join(ROOT, "configs", "voxel18_aspp_nusc.yaml"))
    torch.manual_seed(0)
    det = config.instantiate(cfg["model"]).cuda().train()
    det.backbone.use_half_precision(dtype, training=True)
    B, M = 2, 16
    H = W = 1344 // cfg["_out_size_factor"][0]
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
    print(f"[voxel18 training step {dtype}] loss {float(loss):.6f} -> {float(loss2):.6f}")
    assert bool(torch.isfinite(loss2)) and float(loss2) < float(loss)

"""GPU: every node of the 2-D TRAINING graph (reader -> backbone on _MaskedConv3x3Fn / _MaskedConv3x3F32Fn / _MaskedBNActFn -> the checkpointed ASPP ->
CenterHead on x3_conv / dense_bn_act / _SmallKConv3x3Fn -> the fused loss) against fp64, node by node, with TEACHER FORCING: tests/train_graph_ref.py
records what each node of the real graph received and produced, forward and backward, pushes exactly those operands through the fp64 statement of that
one node and holds the node's recorded outputs to it.  No error carries from node to node, so the bars of tests/test_gpu_train_kernels_at_scale.py apply
unchanged to every node of the COMPOSED graph (test_gpu_decode.py::test_training_graph_on_the_fused_masked_bn_kernels compares whole graphs, and a freshly
initialised net amplifies any rounding difference 1e4 .. 1e5 times from end to end: its bars cannot see a mistake at a minority of sites or in one tensor).

Geometry: that of tests/test_gpu_fused_graph_vs_fp64.py -- 136 x 208 cells of 0.2 m, B = 3 with the middle sample wholly outside the range, the clouds
of its FRAMES[0]: every stage (208/104/52/26 wide, 136/68/34/17 high) has a ragged last tile row and column and the stride-2 data gradient an odd
output height at stage 3.  BatchNorm parameters and running statistics randomised (fresh ones hide gamma / beta mix-ups and the re-centring),
channels_last, labels as test_gpu_decode.py::test_training_step_end_to_end (6 positives per sample).

Three parametrisations, one forward and one backward of model(ex) each: bf16 (autocast; BF_REL, BF_OUT), x3 (fp32, PNX_TRAIN_F32_PIECES=2; X3_REL, X3_FRO)
and x6 (PNX_TRAIN_F32_PIECES=3; X6_REL, X6_FRO); BN_REL for every BatchNorm node; all imported from the at-scale module.
  routing      asserted first: every 3x3 backbone layer, pre_conv's two convolutions, the dilation-1 ASPP branch and every SepHead first convolution carry the
               convolution node's grad_fn, every BN + ReLU (backbone, mapping, neck, shared, deblock, branches) _MaskedBNActFnBackward, every SepHead output
               convolution _SmallKConv3x3FnBackward: CONV_NODES / BN_NODES / SMALLK_NODES.  A layer that fell back to the vendor library fails here;
  wiring       exact (train_graph_ref.check_graph): the mask chain, "output of k = input of k + 1", residuals, upstream gradients, forks (exact for two
               consumers, (n - 1) roundings for n), bit-zero at inactive sites, .grad = what the node returned, the ASPP weight's four uses, the canvas
               gradient the reader's backward received;
  values       per node and element: y, dx, dW, db, dgamma, dbeta, running statistics (two updates inside the checkpointed neck).  The library layers get
               X3_REL (fp32 graphs) or BF_REL + BF_OUT (bf16): a wrong layer, not a rounding regression.  One of them measured above its bar: the fp32 data
               gradient of the one-channel SepHead output convolutions on the vendor library, up to 11.9 x X3_REL of the element's own sum|terms| (7.2e-4)
               at 8.8e-8 relative Frobenius -- a transform-domain kernel's round-off scales with its tile, so that gradient is held to X3_REL x
               train_graph_ref.tile_terms and X3_FRO, and the ratio to the element's own terms is printed (CHANGELOG.md);
  determinism  x3: a second forward + backward from the same state, every recorded HIP-node output and gradient bit-identical.
While the statements run, every `lib` of the package raises.  -rP prints, per node, worst |error| / bar, the Frobenius figures and the ambiguous-gate share."""
import copy

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import train_graph_ref as T  # noqa: E402
from test_gpu_fused_graph_vs_fp64 import B, FRAMES, NX, NY, PC_RANGE, VOXEL, _block_kernels, _frame  # noqa: E402

# nodes per kind: 20 backbone + pre_conv 2 + ASPP d1 + 12 SepHead first convolutions; 21 masked (backbone 20, mapping) + 18 dense (pre_conv 2, post_conv,
# shared, deblock 2, branches 12) BatchNorm nodes; 12 SepHead output convolutions
CONV_NODES, BN_NODES, SMALLK_NODES = 35, 39, 12
HIP_FNS = ("_MaskedConv3x3FnBackward", "_MaskedConv3x3F32FnBackward", "_MaskedBNActFnBackward", "_SmallKConv3x3FnBackward")


def _example(pts):
    H, W, M = NY // 4, NX // 4, 16
    gen = torch.Generator(device="cuda").manual_seed(3)
    ex = {"points": pts, "batch_size": B, "hm": [], "ind": [], "mask": [], "cat": [], "anno_box": [], "gt_boxes": []}
    for names in T.TASKS:
        ex["hm"].append(torch.rand((B, len(names), H, W), device="cuda", generator=gen) * 0.2)
        ex["ind"].append(torch.randint(0, H * W, (B, M), device="cuda", generator=gen))
        m = torch.zeros((B, M), dtype=torch.uint8, device="cuda")
        m[:, :6] = 1
        ex["mask"].append(m)
        ex["cat"].append(torch.randint(0, len(names), (B, M), device="cuda", generator=gen))
        ex["anno_box"].append(torch.randn((B, M, 10), device="cuda", generator=gen) * 0.3)
        ex["gt_boxes"].append(torch.rand((B, M, 7), device="cuda", generator=gen) + torch.tensor([0, 0, -1, 1.5, 0.6, 1.2, 0], device="cuda"))
    return ex


def _step(model, ex, mode, monkeypatch):
    """one forward and one backward of model(ex) under the recorder"""
    for p in model.parameters():
        p.grad = None
    with monkeypatch.context() as mp:
        rec = T.Recorder(model).install(mp)
        try:
            with torch.utils.checkpoint.set_checkpoint_early_stop(False), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode.amp):
                loss, _ = model(ex)
            assert bool(torch.isfinite(loss))
            loss.backward()
        finally:
            rec.remove()
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("prec", ["bf16", "x3", "x6"])
def test_every_node_of_the_training_graph_against_fp64(prec, monkeypatch):
    assert (T.PC_RANGE, T.VOXEL, T.NY, T.NX, T.B, T.CLOUDS) == (PC_RANGE, VOXEL, NY, NX, B, FRAMES[0])
    torch.backends.cudnn.deterministic = True
    if prec != "bf16":
        monkeypatch.setenv("PNX_TRAIN_F32_PIECES", "2" if prec == "x3" else "3")
    mode = T.Mode(prec)
    model = T.build_model().cuda().train().to(memory_format=torch.channels_last)
    assert [int(v) for v in model.reader.grid_size] == [NY, NX]
    pts = _frame(*FRAMES[0])
    assert torch.equal(pts.cpu(), torch.from_numpy(T.cloud_points())), "train_graph_ref.cloud_points is not FRAMES[0]"
    ex = _example(pts)
    state = copy.deepcopy(model.state_dict())
    rec = _step(model, ex, mode, monkeypatch)
    ck = T.Checker(mode)
    want = {mode.conv_fn: CONV_NODES, "_MaskedBNActFnBackward": BN_NODES, "_SmallKConv3x3FnBackward": SMALLK_NODES}
    with monkeypatch.context() as mp:
        _block_kernels(mp)
        # routing first
        have = {}
        for n in rec.nodes.values():
            have[n.gfn] = have.get(n.gfn, 0) + 1
        print(f"[{prec}] grad_fn types of the recorded nodes: {have}")
        assert {k: have.get(k, 0) for k in want} == want, (have, want)
        rec.after_backward(ck)
        occ = rec.occ.unsqueeze(1).float()
        mine = T.cloud_occupancy(T.cloud_points()).cuda()
        ck.need(float(occ[1].sum()) == 0 and float((occ - mine).abs().sum()) <= 0.005 * float(occ.sum()), prec, "the CPU gate test's occupancy is not the reader's",
                float((occ - mine).abs().sum()), float(occ.sum()))
        ck.need(T.zero_bits(rec.canvas.permute(0, 2, 3, 1)[rec.occ == 0]), prec, "canvas not zero off the occupancy")
        first_dx = T.check_graph(ck, model, rec, mode, rec.canvas, occ, counts=want)
        ck.need(len(rec.canvas_grad) == 1 and first_dx is not None and T.biteq(rec.canvas_grad[0], first_dx), prec,
                "the canvas gradient the reader's backward received is not what the first backbone node returned")
        print(f"[{prec}] stage-0 active sites {int(occ.sum())}, per sample {[int(occ[b].sum()) for b in range(B)]}")
    if prec == "x3":
        model.load_state_dict(state)
        again = _step(model, ex, mode, monkeypatch)
        n_cmp = 0
        for key, a in rec.nodes.items():
            b = again.nodes.get(key)
            ck.need(b is not None, key, "not recorded in the second run")
            if b is None or a.gfn not in HIP_FNS:
                continue
            ck.need(T.biteq(a.out, b.out), key, "output differs between two runs from the same state")
            for name in a.expect:
                ck.need(T.biteq(a.grad(name), b.grad(name)), key, name, "gradient differs between two runs from the same state")
                n_cmp += 1
        ck.need(n_cmp > 200, "determinism", "too few tensors compared", n_cmp)
        print(f"[x3] second run from the same state: {n_cmp} gradients and {CONV_NODES + BN_NODES + SMALLK_NODES} outputs of HIP nodes compared bit for bit")
    ck.done(prec)

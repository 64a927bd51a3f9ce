"""CPU: tests/fused_graph_ref.py (the fp64 statement the fused inference graph is held to, layer by layer, in test_gpu_fused_graph_vs_fp64.py) against the
detector's own modules in fp64, where they run torch: the chain of statement functions from a random masked canvas to the head maps must BE
backbone.forward_dense -> neck -> head up to fp64 round-off, with exactly the same masks.  Also: the once-rounded variant really rounds, and
sum|terms| bounds |ref| everywhere."""
import pytest

torch = pytest.importorskip("torch")

import fused_graph_ref as R  # noqa: E402

TASKS = [["car"], ["truck", "bus"]]
RTOL = 1e-10      # of the map's scale: fp64 round-off over <= 2304-term sums in two summation orders


def random_bn_(model, seed):
    """non-trivial BN statistics and affine parameters everywhere (the ranges of test_fused_inference_graph_matches_module_graph)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                for t, lo, hi in ((m.running_mean, -0.2, 0.2), (m.running_var, 0.5, 1.5), (m.weight, 0.6, 1.4), (m.bias, -0.2, 0.2)):
                    t.copy_(torch.empty(t.shape).uniform_(lo, hi, generator=g))


@pytest.fixture(scope="module")
def det():
    from pillarnext_amd.models import build_pillarnext_b

    torch.manual_seed(11)
    model = build_pillarnext_b((-4.0, -2.4, -5.0, 4.0, 2.4, 3.0), (0.2, 0.2, 8.0), tasks=TASKS, with_iou_head=True).eval()
    random_bn_(model, 12)
    return model.double()


@pytest.fixture(scope="module")
def canvas():
    """(B,64,24,40) canvas, zero off the occupancy; the middle sample empty"""
    g = torch.Generator().manual_seed(13)
    mask = (torch.rand((3, 1, 24, 40), generator=g) < 0.15).double()
    mask[1] = 0
    return torch.randn((3, 64, 24, 40), generator=g, dtype=torch.float64) * mask, mask


def _chain(det, x, mask, rounded=None):
    """the statement functions, layer after layer -> every Layer in graph order, the head's as {(task, branch): Layer}"""
    layers = []
    for blk in det.backbone.blocks:
        layers.append(R.sparse_conv_block(blk[0], x, mask, rounded))
        x, mask = layers[-1].ref, layers[-1].mask
        for rb in list(blk)[1:]:
            layers.append(R.sparse_basic_block(rb, x, mask, rounded))
            x = layers[-1].ref
    layers.append(R.mapping(det.backbone, x, mask, rounded))
    layers.append(R.pre_conv(det.neck.pre_conv, layers[-1].ref, rounded))
    layers.append(R.aspp(det.neck, layers[-1].ref, rounded))
    head = R.head(det.head, layers[-1].ref, rounded)
    return layers, {(ti, k): v for ti, d in enumerate(head) for k, v in d.items()}


def _close(tag, a, b):
    scale = float(b.abs().max())
    assert a.shape == b.shape and scale > 0, tag
    assert float((a - b).abs().max()) <= RTOL * scale, (tag, float((a - b).abs().max()), scale)


def test_the_statement_is_the_module_graph(det, canvas):
    x, mask = canvas
    with torch.no_grad():
        layers, head = _chain(det, x, mask)
        # the modules, stage by stage, so that every mask and every stage output is held, not only the end of the chain
        xm, mm, i = x, mask, 0
        for blk in det.backbone.blocks:
            for m in blk:
                xm, mm = m(xm, mm)
                assert torch.equal(layers[i].mask, mm), ("mask", i)
                _close(("backbone layer", i), layers[i].ref, xm)
                assert int(torch.count_nonzero(layers[i].ref * (1 - mm))) == 0
                i += 1
        assert mm.shape[2:] == (3, 5) and float(mm[1].sum()) == 0 and float(mm[0].sum()) > 0
        want = det.backbone.forward_dense(x, mask)
        _close("mapping", layers[i].ref, want)
        assert torch.equal(layers[i].mask, mm)
        _close("pre_conv", layers[i + 1].ref, det.neck.pre_conv(want))
        want = det.neck(want)
        _close("neck", layers[i + 2].ref, want)
        _close("neck (one call)", R.neck(det.neck, layers[i].ref).ref, want)
        preds = det.head(want)
        assert len(preds) == len(TASKS)
        for ti, d in enumerate(preds):
            assert list(d) == ["reg", "height", "dim", "rot", "vel", "iou", "hm"]
            for k, v in d.items():
                _close(("head", ti, k), head[ti, k].ref, v)
        assert head[1, "hm"].ref.shape[1] == 2 and head[0, "hm"].ref.shape[2:] == (6, 10)


def test_the_distributed_aspp_is_the_module_aspp(det, canvas):
    """the form the bars and the once-rounded statement of the neck are taken on equals the module's form"""
    g = torch.Generator().manual_seed(14)
    x = torch.randn((2, 256, 5, 9), generator=g, dtype=torch.float64).relu()
    with torch.no_grad():
        wds, shift = R.aspp_distributed(det.neck)
        y = sum(R.conv2d(x, w, 1, d, d) for w, d in zip(wds, R.ASPP_DILATIONS)) + shift.view(1, -1, 1, 1)
        _close("aspp", torch.relu(y), R.aspp(det.neck, x).ref)


def test_the_rounded_variant_rounds(det, canvas):
    """same input, rounded=dtype: every layer differs from the unrounded statement, by no more than the roundings allow, and holds values of dtype"""
    x, mask = canvas
    with torch.no_grad():
        layers, head = _chain(det, x, mask)
        for dtype in (torch.bfloat16, torch.float16):
            lr, hr = _chain(det, x, mask, rounded=dtype)
            for tag, a, b in [(i, a, b) for i, (a, b) in enumerate(zip(lr, layers))] + [(k, hr[k], head[k]) for k in head]:
                assert torch.equal(a.ref, a.ref.to(dtype).double()), (tag, "not a value of", dtype)
                assert not torch.equal(a.ref, b.ref), (tag, "the rounded variant is a no-op")
                assert a.mask is None or torch.equal(a.mask, b.mask), tag
            assert torch.equal(lr[0].terms, layers[0].terms)             # the bar is that of the unrounded operands
        # one layer on the unrounded input: within (weight + output rounding) of the unrounded statement, and the convolution's own rounding adds to it
        blk = det.backbone.blocks[1][0]                                   # layers[0..2]: stage 0, layers[11]: the last block of stage 3
        xin, min_ = layers[2].ref, layers[2].mask
        u, r = R.sparse_conv_block(blk, xin, min_), R.sparse_conv_block(blk, xin, min_, rounded=torch.bfloat16)
        h = 2.0 ** -9                                                     # half an ulp of bf16: the weights, then the output
        assert float(((r.ref - u.ref).abs() - (h * (1 + h) * u.terms + h * u.ref.abs())).max()) <= 0
        m0 = R.mapping(det.backbone, layers[11].ref, layers[11].mask, rounded=torch.bfloat16)
        m1 = R.mapping(det.backbone, layers[11].ref, layers[11].mask, rounded=torch.bfloat16, conv_out=True)
        assert not torch.equal(m0.ref, m1.ref)


def test_sum_of_terms_bounds_the_statement(det, canvas):
    x, mask = canvas
    with torch.no_grad():
        layers, head = _chain(det, x, mask)
    for tag, l in list(enumerate(layers)) + list(head.items()):
        assert bool((l.terms * (1 + 1e-12) >= l.ref.abs()).all()), tag
        assert float(l.terms.max()) > 0
    nk = layers[-1]
    assert nk.parts is not None and bool((nk.parts + nk.terms >= nk.ref).all())

"""CPU: the launch schedule of models.FusedPillarNeXt, pinned to the commit before its two copies (Python loop / launch plan) became one walk.

Part a canonicalises the launch tables of the backbone and of the lazy head (kind, the used ints, every pointer replaced by the index of its
first appearance in the table, the Dyn slots by name); part b runs forward_preds with every ops.* launch replaced by a fake that allocates a
tensor of the right shape and logs the call (shapes, scalars, which arguments are None, tensor identities by first appearance).  Order,
buffer rotation, residual wiring, tile-list sharing and the stride-2 `tiles=None` all show in either.  Nothing varies from run to run.

tests/golden/fused_schedule.json was written at that commit by this module's own helpers, from the repository root:

    import json, sys
    sys.path.insert(0, "tests")
    import test_fused_schedule_cpu as t
    from pillarnext_amd._lib import PnxError

    def head_plan(fused, x):          # the table was only reachable through the call that also ran it
        try:
            fused._run_head_plan(x)
        except PnxError:              # run() refuses CPU tensors; the frozen plan is cached by then
            pass
        return next(v for k, v in fused._ws.items() if isinstance(k, tuple) and k[0] == "plan_head")

    json.dump({"tables": t.tables(head_plan), "traces": t.traces()}, open(t.GOLDEN, "w"), indent=1)
"""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_schedule.json")
B = 2
N_INTS = {1: 4, 2: 5, 3: 8, 4: 7, 5: 5}   # plan.OP_*: the entries of pnx_op.i a call of that kind uses


def model():
    from pillarnext_amd.models import FusedPillarNeXt, build_pillarnext_b

    torch.manual_seed(5)
    det = build_pillarnext_b((-6.4, -7.2, -5.0, 6.4, 7.2, 3.0), (0.2, 0.2, 8.0), tasks=[["car"], ["truck", "bus"]], with_iou_head=True).eval()
    fused = FusedPillarNeXt(det, hip_conv=True)
    assert [int(v) for v in fused.reader.grid_size] == [72, 64] and fused.lazy_head
    return fused


def _nhwc(b, c, h, w):
    return torch.zeros((b, c, h, w), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _occupancy(ny, nx):
    occ = torch.zeros((B, ny, nx), dtype=torch.uint8)
    occ[:, 3::7, 5::11] = 1
    return occ


# ---------------------------------------------------------------------------------------------- part a: launch tables
def canonical(plan):
    seen, rows = {}, []
    for k in range(len(plan)):
        op = plan._arr[k]
        rows.append([op.kind, list(op.i[:N_INTS[op.kind]]), [None if p is None else seen.setdefault(p, len(seen)) for p in op.p]])
    return {"ops": rows, "dyn": sorted([k, j, name] for name, (_, where) in plan._dyn.items() for k, j in where)}


def tables(head_plan):
    fused = model()
    bb = fused._backbone_plan(B, torch.device("cpu"))
    assert {"canvas", "occ", "plan", "out", "mask"} <= set(bb) and fused._ws[("plan_bb", B, torch.device("cpu"))] is bb
    head = head_plan(fused, _nhwc(B, 256, 9, 8))
    return {"backbone": canonical(bb["plan"]), "backbone_out": [list(bb["out"].shape), list(bb["mask"].shape)], "head": canonical(head)}


# ---------------------------------------------------------------------------------------------- part b: eager trace
class Trace:
    def __init__(self):
        self.calls, self._ids, self._keep = [], {}, []

    def ident(self, t):
        """Tensors by first appearance (kept alive, so that no id() comes back); tuples / lists element by element."""
        if t is None:
            return None
        if isinstance(t, (tuple, list)):
            return [self.ident(v) for v in t]
        self._keep.append(t)
        return [self._ids.setdefault(id(t), len(set(self._ids.values()))), list(t.shape)]

    def log(self, name, result, scalars=(), **tensors):
        self.calls.append([name, {k: self.ident(v) for k, v in tensors.items()}, list(scalars), self.ident(result)])
        return result

    def patch(self, mp):
        from pillarnext_amd import ops

        def hw(h, w, stride):
            return (h - 1) // stride + 1, (w - 1) // stride + 1

        def mask_pool3(mask, stride):
            b, h, w = mask.shape
            return self.log("mask_pool3", torch.zeros((b, *hw(h, w, stride)), dtype=torch.uint8), [stride], mask=mask)

        def conv_tile_list(mask, dirties, tile_rows, out=None):
            b, h, w = mask.shape
            got = out
            if out is None:
                out = (torch.zeros((b * ((h + tile_rows - 1) // tile_rows) * ((w + 31) // 32),), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32))
            return self.log("conv_tile_list", out, [tile_rows], mask=mask, dirties=dirties, out=got)

        def conv3x3_masked(x, wfrag, bias, cout, stride=1, mask=None, residual=None, relu=True, out=None, tiles=None):
            b, _, h, w = x.shape
            y = out[0] if out is not None else _nhwc(b, cout, *hw(h, w, stride))
            return self.log("conv3x3_masked", y, [cout, stride, relu], x=x, wfrag=wfrag, bias=bias, mask=mask, residual=residual, out=out, tiles=tiles)

        def deconv2x2(x, wfrag, bias, cout, relu=True):
            b, _, h, w = x.shape
            return self.log("deconv2x2", _nhwc(b, cout, 2 * h, 2 * w), [cout, relu], x=x, wfrag=wfrag, bias=bias)

        def sephead_out(x, wfrag, bias):
            b, _, h, w = x.shape
            return self.log("sephead_out", _nhwc(b, 16, h, w), x=x, wfrag=wfrag, bias=bias)

        def bias_act_mask_(x, bias, mask=None, residual=None, relu=True):
            return self.log("bias_act_mask_", x, [int(relu)], x=x, bias=bias, mask=mask, residual=residual)

        def sum_bias_act(parts, bias, relu=True):
            return self.log("sum_bias_act", torch.zeros_like(parts[0]), [relu], parts=parts, bias=bias)

        for f in (mask_pool3, conv_tile_list, conv3x3_masked, deconv2x2, sephead_out, bias_act_mask_, sum_bias_act):
            mp.setattr(ops, f.__name__, f)


def _with_reader(mp, fused, tr):
    """forward_dense replaced: the canvas and the occupancy of a fixed pattern, first in the trace's numbering."""
    ny, nx = (int(v) for v in fused.reader.grid_size)
    canvas, occ = _nhwc(B, 64, ny, nx), _occupancy(ny, nx)
    tr.ident(canvas), tr.ident(occ)

    def forward_dense(points, batch_size, dtype=torch.bfloat16, out=None, occupancy=None):
        assert out is None and batch_size == B and dtype == torch.bfloat16
        occupancy.copy_(occ)
        tr._ids[id(occupancy)] = tr._ids[id(occ)]     # the model allocates the occupancy it hands the reader
        tr._keep.append(occupancy)
        return canvas

    mp.setattr(fused.reader, "forward_dense", forward_dense)
    return canvas, occ


SETTINGS = {   # name: (sparse_ws, lazy, packed_out?, taps?)
    "lazy_packed": (True, True, True, False),
    "dense_packed": (True, False, True, False),
    "no_workspaces": (False, None, False, True),
}


def trace(name, mp):
    sparse_ws, lazy, want_packed, want_taps = SETTINGS[name]
    fused, tr = model(), Trace()
    fused.use_plan, fused.sparse_ws = False, sparse_ws
    tr.patch(mp)
    _with_reader(mp, fused, tr)
    packed, taps = ([] if want_packed else None), ({} if want_taps else None)
    preds = fused.forward_preds(torch.zeros((1, 6)), B, packed_out=packed, taps=taps, lazy=lazy)
    res = {"calls": tr.calls, "preds": [{k: tr.ident(v)[1] for k, v in d.items()} for d in preds]}
    if packed is not None:
        res["packed"] = [[type(p).__name__, tr.ident([p.dense, p.up] if hasattr(p, "up") else p)] for p in packed]
    if taps is not None:
        res["taps"] = {k: tr.ident(v) for k, v in taps.items()}
    return res


def traces():
    out = {}
    for name in SETTINGS:
        with pytest.MonkeyPatch.context() as mp:
            out[name] = trace(name, mp)
    return out


# ---------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _plain(v):
    return json.loads(json.dumps(v))


def test_planned_tables_equal_the_recorded_schedule(golden):
    got = _plain(tables(lambda fused, x: fused._head_plan(x)))
    for k in ("backbone", "backbone_out", "head"):
        assert got[k] == golden["tables"][k], k


@pytest.mark.parametrize("name", list(SETTINGS))
def test_eager_trace_equals_the_recorded_schedule(golden, name, monkeypatch):
    got = _plain(trace(name, monkeypatch))
    want = golden["traces"][name]
    assert len(got["calls"]) == len(want["calls"])
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {k}"
    assert got == want


def test_backbone_walk_runs_without_the_reader(golden, monkeypatch):
    """The walk takes the canvas and the mask as arguments: driven directly, it issues the calls forward_preds issues up to the mapping conv."""
    fused, tr = model(), Trace()
    fused.use_plan = False
    tr.patch(monkeypatch)
    ny, nx = (int(v) for v in fused.reader.grid_size)
    canvas, occ = _nhwc(B, 64, ny, nx), _occupancy(ny, nx)
    tr.ident(canvas), tr.ident(occ)
    x, mask = fused._backbone(canvas, occ)
    want = golden["traces"]["lazy_packed"]["calls"]
    n = next(k for k, c in enumerate(want) if c[0] == "bias_act_mask_")
    assert _plain(tr.calls) == want[:n] and n == len(tr.calls)
    assert [tr.ident(x), tr.ident(mask)] == [want[n - 1][3], want[n - 1][1]["mask"]]

"""CPU: what the split of models.py into train_nodes.py (training nodes and routing), fused.py (the fused inference graph) and switches.py
(the table of environment switches) must keep: the fused model's buffers bit for bit, the layering of the new modules, the public names of
pillarnext_amd.models, the switch reader's rules, and that the masked-BatchNorm wrappers of ops.py reject bad operands before the library is entered.

tests/golden/fused_state.json was written at the commit before the split by this module's own helper, from the repository root:

    import json, sys
    sys.path.insert(0, "tests")
    import test_models_split_cpu as t
    json.dump(t.fused_state(), open(t.GOLDEN, "w"), indent=0)
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "fused_state.json")


# ---------------------------------------------------------------------------------------------- 1: the fused model's state, bit for bit
def fused_state():
    """Every state_dict() entry of test_fused_schedule_cpu.model() in order: [name, shape, dtype, SHA-256 of its bytes]."""
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    from test_fused_schedule_cpu import model

    rows = []
    for name, t in model().state_dict().items():
        raw = t.detach().cpu().contiguous().flatten().view(torch.uint8).numpy().tobytes()
        rows.append([name, list(t.shape), str(t.dtype), hashlib.sha256(raw).hexdigest()])
    return rows


def test_fused_weights_are_bit_identical():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = fused_state()
    assert len(want) == 242 and [r[0] for r in got] == [r[0] for r in want]
    for g, w in zip(got, want):
        assert g == w, g[0]


# ---------------------------------------------------------------------------------------------- 2: layering
def _loaded_after(*names):
    """Per name, the pillarnext_amd modules in sys.modules after `import pillarnext_amd.<name>` in a fresh interpreter (the children run side by side)."""
    code = "import pillarnext_amd.{}, sys; print(' '.join(m for m in sys.modules if m.startswith('pillarnext_amd.')))"
    children = [subprocess.Popen([sys.executable, "-c", code.format(n)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for n in names]
    for p in children:
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, err[-2000:]
        yield {m.split(".", 1)[1] for m in out.split()}


def test_layering():
    nodes, fused, models = _loaded_after("train_nodes", "fused", "models")
    assert {"train_nodes", "ops", "switches", "dist_utils"} <= nodes and not nodes & {"models", "reader", "fused"}, nodes
    assert {"fused", "ops", "plan", "switches"} <= fused and not fused & {"models", "reader", "train_nodes"}, fused
    assert {"models", "train_nodes", "fused", "switches"} <= models, models


# ---------------------------------------------------------------------------------------------- 3: the surface of pillarnext_amd.models
HOMES = {"fused": ("FusedPillarNeXt", "fold_aspp", "LazyTask"),
         "train_nodes": ("masked_conv", "masked_bn_act", "dense_bn_act", "x3_conv", "x3_ok", "smallk_conv", "split_f32_pieces", "train_f32_pieces")}
STAY = ("_spconv_weight_to_conv2d", "_SpConv2d", "MaskedBatchNorm", "convert_sync_batchnorm", "SparseConvBlock", "SparseBasicBlock", "SparseResNet",
        "ASPPNeck", "SepHead", "CenterHead", "SingleStageDetector", "_task_nms", "NUSC_TASKS", "build_pillarnext_b")


def test_surface():
    import importlib

    from pillarnext_amd import models

    for home, names in HOMES.items():
        mod = importlib.import_module("pillarnext_amd." + home)
        for name in names:
            assert getattr(models, name) is getattr(mod, name), name
    for name in STAY:
        assert hasattr(models, name), name
    assert models.FusedPillarNeXt.__module__ == "pillarnext_amd.fused"
    assert models.SingleStageDetector.__module__ == "pillarnext_amd.models"


MOVED_PRIVATE = {"fused": ("_fold_bn", "_FusedConv", "_HipConv3x3", "_HipDeconv2x2", "_HipSepHeadOut", "_DeferredDecode"),
                 "train_nodes": ("_MaskedBNActFn", "_MaskedConv3x3Fn", "_MaskedConv3x3F32Fn", "_SmallKConv3x3Fn", "_split_pack", "bf16_dense_ok")}


def test_moved_private_names_still_resolve_through_models():
    """What older code and pickles written before the split name as pillarnext_amd.models.<name>: the same objects, by attribute and by import."""
    import importlib
    import pickle

    from pillarnext_amd import models
    from pillarnext_amd.models import _fold_bn, _HipConv3x3, _split_pack  # noqa: F401

    for home, names in MOVED_PRIVATE.items():
        mod = importlib.import_module("pillarnext_amd." + home)
        for name in names:
            assert getattr(models, name) is getattr(mod, name), name
    with pytest.raises(AttributeError):
        models._no_such_name
    # a pickle from before the split refers to the layer classes by their old module: protocol 0 spells the reference out as text
    layer = models._FusedConv(torch.zeros(8, 8, 1, 1), torch.zeros(8))
    old = pickle.dumps(layer, protocol=0).replace(b"cpillarnext_amd.fused\n_FusedConv", b"cpillarnext_amd.models\n_FusedConv")
    assert b"pillarnext_amd.models" in old and type(pickle.loads(old)) is type(layer)


# ---------------------------------------------------------------------------------------------- 4: switches
def test_switch_values(monkeypatch):
    from pillarnext_amd import switches
    from pillarnext_amd._lib import PnxError

    for name, default in (("PNX_TRAIN_HIPCONV", True), ("PNX_HEAD_LAZY_TORCH", False)):
        assert switches.SWITCHES[name][0] is default
        monkeypatch.delenv(name, raising=False)
        assert switches.on(name) is default
        monkeypatch.setenv(name, "0")       # set after the import: nothing is cached
        assert switches.on(name) is False
        monkeypatch.setenv(name, "1")
        assert switches.on(name) is True
        for junk in ("false", "true", "", "2", " 1", "on"):
            monkeypatch.setenv(name, junk)
            with pytest.raises(PnxError, match=name):
                switches.on(name)
    with pytest.raises(KeyError):
        switches.on("PNX_TRAIN_HIPCNOV")
    with pytest.raises(KeyError):           # 2 or 3, not a bool: train_f32_pieces() reads it
        switches.on("PNX_TRAIN_F32_PIECES")
    assert all(isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], str) and v[1] for v in switches.SWITCHES.values())


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _sources(*dirs, ext=(".py",)):
    for d in dirs:
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for fn in files:
                if fn.endswith(ext):
                    yield os.path.join(base, fn)


def test_every_switch_a_test_or_tool_sets_is_read_somewhere():
    from pillarnext_amd import switches

    c_side = set()
    for path in _sources(os.path.join("pillarnext_amd", "csrc"), ext=(".hip", ".h", ".cpp", ".c")):
        c_side |= set(re.findall(r'getenv\("(PNX_[A-Z0-9_]+)"\)', open(path).read()))
    build_side = set(re.findall(r"PNX_[A-Z0-9_]+", _read("pillarnext_amd", "build.py") + _read("bench.py") + _read("__graft_entry__.py")))
    assert len(c_side) >= 5 and "PNX_FORCE_REBUILD" in build_side
    setter = re.compile(r"""(?:setenv\(\s*|os\.environ\[)["'](PNX_[A-Z0-9_]+)["']""")
    me = os.path.abspath(__file__)
    used = {}
    for path in _sources("tests", "tools"):
        if os.path.abspath(path) != me:      # this file sets misspelt names on purpose
            for name in setter.findall(open(path).read()):
                used.setdefault(name, os.path.relpath(path, ROOT))
    assert len(used) >= 10
    stray = {n: p for n, p in used.items() if n not in switches.SWITCHES and n not in c_side and n not in build_side}
    assert not stray, stray


def test_no_direct_environment_reads_are_left():
    for name in ("models", "train_nodes", "fused", "reader", "mvf_encoder", "decode"):
        assert 'os.environ.get("PNX_' not in _read("pillarnext_amd", name + ".py"), name
    src = _read("pillarnext_amd", "models.py")
    for word in ("_Masked", "_Hip", "ctypes", "os.environ"):
        assert word not in src, word
    node = _read("pillarnext_amd", "train_nodes.py")
    node = node[node.index("class _MaskedBNActFn"):node.index("def _mask_u8")]
    for word in ("ctypes", "lib()", "ptr(", "stream_ptr"):
        assert word not in node, word


# ---------------------------------------------------------------------------------------------- 5: the masked-BatchNorm wrappers reject before launching
class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is a CUDA tensor: lets every other operand check be reached, one at a time, on a machine without a GPU."""
    is_cuda = property(lambda self: True)


def _bn_args(shape, dtype=torch.float32, gpu=True):
    """Good operands of the masked_bn_* wrappers for a (B,C,H,W) map, by wrapper name, as dicts name -> value in call order."""
    B, C, H, W = shape

    def t(*size, dtype=torch.float32):
        v = torch.zeros(size, dtype=dtype)
        return v.as_subclass(_OnGpu) if gpu else v

    def fmap():
        m = torch.zeros(shape, dtype=dtype).contiguous(memory_format=torch.channels_last)
        return m.as_subclass(_OnGpu) if gpu else m

    vec = lambda: t(C)    # noqa: E731
    return {
        "masked_bn_stats": dict(x=fmap(), mask=t(B * H * W), center=vec()),
        "masked_bn_reduce": dict(part=t(4, 2 * C + 1)),
        "masked_bn_finalize": dict(sums=t(2 * C + 1, dtype=torch.float64), center=vec(), weight=vec(), bias=vec(), eps=1e-3, momentum=0.01,
                                   running_mean=vec(), running_var=vec(), num_batches_tracked=t(dtype=torch.int64)),
        "masked_bn_apply": dict(x=fmap(), residual=fmap(), mask=t(B * H * W), scale=vec(), shift=vec(), relu=True),
        "masked_bn_bwd_stats": dict(gy=fmap(), x=fmap(), residual=fmap(), mask=t(B * H * W), scale=vec(), shift=vec(), mean=vec(), invstd=vec(), relu=True),
        "masked_bn_bwd_finalize": dict(sums_local=t(2 * C, dtype=torch.float64), sums_global=None, count=t(1)),
        "masked_bn_bwd_apply": dict(gy=fmap(), x=fmap(), residual=fmap(), mask=t(B * H * W), scale=vec(), shift=vec(), mean=vec(), invstd=vec(), relu=True,
                                    mean_g=vec(), mean_gx=vec(), want_residual_grad=True),
    }


WRAPPERS = list(_bn_args((1, 8, 1, 1)))
SHAPE = (2, 64, 5, 7)


@pytest.fixture
def no_library(monkeypatch):
    from pillarnext_amd import ops

    def entered(*a, **k):
        raise AssertionError("the library was entered")

    monkeypatch.setattr(ops, "lib", entered)
    return ops


@pytest.mark.parametrize("name", WRAPPERS)
def test_masked_bn_wrappers_accept_what_the_node_passes(no_library, name):
    """The control of the rejections below: with good operands every wrapper gets as far as the library."""
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(AssertionError, match="the library was entered"):
            getattr(no_library, name)(**_bn_args(SHAPE, dtype)[name])


@pytest.mark.parametrize("name", WRAPPERS)
def test_masked_bn_wrappers_reject_before_launching(no_library, name):
    ops = no_library
    fn = getattr(ops, name)
    good = _bn_args(SHAPE)[name]
    cases = {"cpu tensors": _bn_args(SHAPE, gpu=False)[name], "48 channels": _bn_args((1, 48, 4, 4))[name]}
    if "x" in good:
        nchw = torch.zeros(SHAPE).as_subclass(_OnGpu)
        assert nchw.is_contiguous() and not nchw.is_contiguous(memory_format=torch.channels_last)
        cases["nchw x"] = dict(good, x=nchw)
        cases["bf16 mask"] = dict(good, mask=good["mask"].to(torch.bfloat16).as_subclass(_OnGpu))
        cases["mask of another size"] = dict(good, mask=good["mask"][:-1])
        cases["fp16 x"] = dict(good, x=good["x"].to(torch.float16).as_subclass(_OnGpu))
    if "residual" in good:
        cases["residual of another dtype"] = dict(good, residual=good["residual"].to(torch.bfloat16).as_subclass(_OnGpu))
        cases["residual of another shape"] = dict(good, residual=_bn_args((2, 64, 5, 6))[name]["residual"])
    if "scale" in good:
        cases["fp64 scale"] = dict(good, scale=good["scale"].double().as_subclass(_OnGpu))
        cases["strided shift"] = dict(good, shift=torch.zeros(128).as_subclass(_OnGpu)[::2])
    for what, kw in cases.items():
        with pytest.raises(ops.PnxError):
            fn(**kw)
            pytest.fail(f"{name} accepted {what}")

"""CPU: tests/sync_replay.py itself, and through it the synchronised mode of train_nodes._MaskedBNActFn's torch path (CPU tensors: three collectives,
[sum x | count], [sum (x - mean)^2] forward and [sum g | sum g xhat] backward) at worlds 2 and 3 against the fp64 autograd statement of the JOINT
batch, at the tolerances of test_dist_gloo.py::_worker_syncbn.  No process is started and no collective backend initialised."""
import copy

import pytest

torch = pytest.importorskip("torch")

from sync_replay import Replay, ReplayError  # noqa: E402

C, H, W = 8, 9, 11
EPS, MOM = 1e-3, 0.1


def _inputs(Bs, empty_rank=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = sum(Bs)
    x = torch.randn((n, C, H, W), generator=g) * (torch.rand(C, generator=g) + 0.5).view(1, -1, 1, 1) + torch.randn(C, generator=g).view(1, -1, 1, 1)
    res = torch.randn((n, C, H, W), generator=g)
    gy = torch.randn((n, C, H, W), generator=g)
    dens = 0.2 + 0.4 * torch.rand((n, 1, 1, 1), generator=g)
    mask = (torch.rand((n, 1, H, W), generator=g) < dens).float()
    lo = [sum(Bs[:r]) for r in range(len(Bs))]
    if empty_rank is not None:
        mask[lo[empty_rank]: lo[empty_rank] + Bs[empty_rank]] = 0
    from pillarnext_amd.models import MaskedBatchNorm

    norm = MaskedBatchNorm(C, eps=EPS, momentum=MOM).train()
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(C, generator=g) * 0.3)
        norm.running_mean.copy_(torch.randn(C, generator=g))
        norm.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    # no ReLU gate within rounding of zero: the upstream gradient is zero where the fp64 pre-activation of the joint batch is within 1e-4 of it
    with torch.no_grad():
        m = mask.double()
        cnt = m.sum().clamp(min=1.0)
        mean = (x.double() * m).sum(dim=(0, 2, 3), keepdim=True) / cnt
        var = (((x.double() - mean) ** 2) * m).sum(dim=(0, 2, 3), keepdim=True) / cnt
        pre = (x.double() - mean) / torch.sqrt(var + EPS) * norm.weight.double().view(1, -1, 1, 1) + norm.bias.double().view(1, -1, 1, 1) + res.double()
        gy = gy * (pre.abs() > 1e-4)
    return x, mask, res, gy, norm, lo


def _joint_fp64(x, mask, res, gy, norm):
    """BatchNorm1d over the active sites of the joint batch + residual + ReLU, times the mask; fp64, gradients by autograd"""
    x64, r64 = x.double().requires_grad_(True), res.double().requires_grad_(True)
    gam, bet = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    m = mask.double()
    cnt = m.sum().clamp(min=1.0)
    mean = (x64 * m).sum(dim=(0, 2, 3)) / cnt
    var = (((x64 - mean.view(1, -1, 1, 1)) ** 2) * m).sum(dim=(0, 2, 3)) / cnt
    xhat = (x64 - mean.view(1, -1, 1, 1)) / torch.sqrt(var + norm.eps).view(1, -1, 1, 1)
    y = torch.relu(xhat * gam.view(1, -1, 1, 1) + bet.view(1, -1, 1, 1) + r64) * m
    y.backward(gy.double())
    rm = (1 - MOM) * norm.running_mean.double() + MOM * mean.detach()
    rv = (1 - MOM) * norm.running_var.double() + MOM * (var * cnt / (cnt - 1).clamp(min=1.0)).detach()
    return dict(y=y.detach(), dx=x64.grad, dres=r64.grad, dgamma=gam.grad, dbeta=bet.grad, rm=rm, rv=rv)


def _rank_fn(x, mask, res, gy, norm, lo, Bs):
    from pillarnext_amd.models import masked_bn_act

    def fn(rank, token):
        sl = slice(lo[rank], lo[rank] + Bs[rank])
        n = copy.deepcopy(norm).enable_sync(process_group=token)
        xa, ra = x[sl].clone().requires_grad_(True), res[sl].clone().requires_grad_(True)
        y = masked_bn_act(xa, mask[sl], n, residual=ra, relu=True)
        assert type(y.grad_fn).__name__ == "_MaskedBNActFnBackward"
        y.backward(gy[sl])
        return dict(y=y.detach(), dx=xa.grad, dres=ra.grad, dgamma=n.weight.grad, dbeta=n.bias.grad, rm=n.running_mean, rv=n.running_var,
                    nbt=int(n.num_batches_tracked))
    return fn


@pytest.mark.parametrize("Bs,empty_rank", [([1, 2], None), ([2, 1, 2], 1)])
def test_masked_bn_torch_path_equals_the_joint_batch(Bs, empty_rank):
    x, mask, res, gy, norm, lo = _inputs(Bs, empty_rank)
    ref = _joint_fp64(x, mask, res, gy, norm)
    rp = Replay(len(Bs))
    out = rp.run(_rank_fn(x, mask, res, gy, norm, lo, Bs))
    assert rp.passes == 4 and len(rp.known) == 3                     # three collectives per rank: the fourth pass is exact
    assert [tuple(k.shape) for k in rp.known] == [(C + 1,), (C,), (2 * C,)]
    for r, o in enumerate(out):
        sl = slice(lo[r], lo[r] + Bs[r])
        torch.testing.assert_close(o["y"].double(), ref["y"][sl], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(o["dx"].double(), ref["dx"][sl], rtol=2e-3, atol=2e-4)
        torch.testing.assert_close(o["dres"].double(), ref["dres"][sl], rtol=0, atol=0)
        torch.testing.assert_close(o["rm"].double(), ref["rm"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(o["rv"].double(), ref["rv"], rtol=1e-5, atol=1e-6)
        assert o["nbt"] == 1
    # parameter gradients are the LOCAL sums (DistributedDataParallel averages them): their sum over the ranks is the joint gradient
    for k in ("dgamma", "dbeta"):
        torch.testing.assert_close(sum(o[k].double() for o in out), ref[k], rtol=2e-3, atol=2e-4)
    if empty_rank is not None:
        assert float(out[empty_rank]["y"].abs().max()) == 0.0 and float(out[empty_rank]["dgamma"].abs().max()) == 0.0
    print(f"[sync replay cpu] world {len(Bs)}: passes {rp.passes}, worst |err| " + " ".join(
        f"{k} {max(float((o[k].double() - ref[k][slice(lo[r], lo[r] + Bs[r])]).abs().max()) for r, o in enumerate(out)):.1e}" for k in ("y", "dx", "dres")))


def test_world_1_returns_the_single_process_result():
    """world 1: the local sums ARE the global ones; the harness still walks its L + 1 passes and returns the plain result bit for bit"""
    from pillarnext_amd.models import masked_bn_act

    x, mask, res, gy, norm, lo = _inputs([2])
    rp = Replay(1)
    out = rp.run(_rank_fn(x, mask, res, gy, norm, lo, [2]))[0]
    n = copy.deepcopy(norm)
    xa = x.clone().requires_grad_(True)
    y = masked_bn_act(xa, mask, n, residual=res.clone().requires_grad_(True), relu=True)
    y.backward(gy)
    assert rp.passes == 4
    assert torch.equal(out["y"], y.detach()) and torch.equal(out["dx"], xa.grad) and torch.equal(out["rm"], n.running_mean)


def test_unequal_collective_counts_are_refused():
    from pillarnext_amd import dist_utils

    def fn(rank, token):
        t = torch.ones(3)
        dist_utils.all_reduce_sum(t, token)
        if rank == 1:                                                # a rank that issues one more: the others would never answer it
            dist_utils.all_reduce_sum(t, token)
        return t

    with pytest.raises(ReplayError, match="would hang"):
        Replay(2).run(fn)


def test_unequal_shapes_and_dtypes_are_refused():
    from pillarnext_amd import dist_utils

    with pytest.raises(ReplayError, match="disagree on the tensor"):
        Replay(2).run(lambda rank, token: dist_utils.all_reduce_sum(torch.ones(3 + rank), token))
    with pytest.raises(ReplayError, match="dtype"):
        Replay(2).run(lambda rank, token: dist_utils.all_reduce_sum(torch.ones(3, dtype=torch.float64 if rank else torch.float32), token))


def test_a_foreign_group_is_refused():
    from pillarnext_amd import dist_utils

    with pytest.raises(ReplayError, match="not the group given"):
        Replay(2).run(lambda rank, token: dist_utils.all_reduce_sum(torch.ones(3), None))


def test_a_contribution_that_changes_between_passes_is_refused():
    from pillarnext_amd import dist_utils

    calls = [0]

    def fn(rank, token):
        calls[0] += 1
        a = torch.full((2,), float(rank + 1))
        if rank == 0:
            a[0] += 1e-3 * calls[0]                                  # deliberately not a function of the inputs
        dist_utils.all_reduce_sum(a, token)
        b = a * 2
        dist_utils.all_reduce_sum(b, token)
        return b

    with pytest.raises(ReplayError, match="differs from the pass before"):
        Replay(2).run(fn)


def test_the_exact_pass_sees_the_sums_and_the_patch_is_undone():
    from pillarnext_amd import dist_utils

    before = dist_utils.all_reduce_sum

    def fn(rank, token):
        a = torch.tensor([1.0 + rank, 10.0])
        dist_utils.all_reduce_sum(a, token)                          # [1 + 2 + 3, 30]
        b = a * (rank + 1)
        dist_utils.all_reduce_sum(b, token)                          # (1 + 2 + 3) * [6, 30]
        return a, b

    rp = Replay(3)
    out = rp.run(fn)
    assert rp.passes == 3
    for a, b in out:
        assert a.tolist() == [6.0, 30.0] and b.tolist() == [36.0, 180.0]
    assert dist_utils.all_reduce_sum is before
    with pytest.raises(ReplayError):                                 # also after a failing pass
        Replay(2).run(lambda rank, token: dist_utils.all_reduce_sum(torch.ones(1 + rank), token))
    assert dist_utils.all_reduce_sum is before


@pytest.mark.parametrize("name", ["world2", "world3_middle_out_of_range", "world2_rank1_no_rows"])
def test_joint_reader_cases_of_the_gpu_module_meet_the_twins_conditions(name):
    """The joint clouds of test_gpu_sync_nodes_vs_fp64.py, built here on the host: the caps of pfn_train_ref.conditions hold (asserted when the case
    is built), every joint pillar lies in exactly one rank's frames, and the ranks the cases are there for hold no pillar."""
    import numpy as np

    from test_gpu_sync_nodes_vs_fp64 import PFN_WORLDS, pfn_world

    assert set(PFN_WORLDS) == {"world2", "world3_middle_out_of_range", "world2_rank1_no_rows"}
    w = pfn_world(name)
    s, Bs, lo = w["c"]["ref"], w["Bs"], w["lo"]
    per_rank = [int(((s["coords"][:, 0] >= lo[r]) & (s["coords"][:, 0] < lo[r] + Bs[r])).sum()) for r in range(len(Bs))]
    assert sum(per_rank) == s["P"] and s["N"] <= sum(len(p) for p in w["clouds"])
    if name == "world2":
        assert Bs == [1, 2] and len({len(p) for p in w["clouds"]}) == 2 and min(per_rank) > 1000
    elif name == "world3_middle_out_of_range":
        assert per_rank[1] == 0 and len(w["clouds"][1]) > 0 and min(per_rank[0], per_rank[2]) > 1000
    else:
        assert per_rank[1] == 0 and w["clouds"][1].shape == (0, 6)
    assert np.array_equal(np.sort(w["keys"]), w["keys"]) and len(np.unique(w["keys"])) == s["P"]

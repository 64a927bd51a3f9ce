"""GPU: the synchronised (world > 1) mode of the two hand-written BatchNorm paths against the fp64 statement of the JOINT batch:

  train_nodes._MaskedBNActFn on csrc/masked_bn.hip (masked_bn_act, PNX_MASKED_BN_HIP=1): one forward and one backward collective;
  pfn_train.FusedPFNTrain on csrc/pfn_train.hip (PNX_TRAIN_FUSED=1): two forward and two backward collectives.

World N runs in this one process, rank after rank, through tests/sync_replay.py (no process started, no collective backend initialised): the
k-th collective of a rank receives the fp64 sum of every rank's k-th contribution, as an all-reduce would deliver it.  tests/test_gpu_dist.py holds
the same nodes to rtol 5e-3 in separate processes at one geometry; here every quantity is held to the bars of the single-rank fp64 tests
(test_gpu_train_kernels_at_scale.py::test_masked_bn_*, test_gpu_pfn_train_vs_fp64.py), so that what is specific to the mode shows: a local sum
where the global one belongs or the reverse (dgamma / dbeta are LOCAL sums, the two means of dx global), the global count in the unbiased variance,
a rank with no active site or exactly one, three ranks of unequal size, a rank without a pillar or without a point, and running means that differ
between the ranks (the statistics of a batch must not depend on the buffers).

-rP prints worst |error| / bar of every quantity."""
import copy
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pfn_train_ref as T  # noqa: E402
from sync_replay import Replay  # noqa: E402
from test_gpu_pfn_train_vs_fp64 import GRADS, make_net  # noqa: E402  (momentum 1, zero running statistics: they ARE the batch statistics)
from test_gpu_train_kernels_at_scale import BF_OUT, BN_REL, _bn_ref, _bn_ref_backward, _check, _cl  # noqa: E402  (the single-rank statement and its bars, unchanged)

H, W = 37, 53
# momentum 0.1, not the model's 0.01: a rank of one map holds ~800 of the ~2 400 active sites, so the LOCAL count in the unbiased variance would move
# running_var by momentum * var * (1/799 - 1/2399) = 8e-5 var at 0.1 -- four times its bar of 2^-16 (1 + 2 momentum) var -- but by only half the bar at 0.01
EPS, MOM = 1e-3, 0.1


# ---------------------------------------------------------------------------------------------------- masked BatchNorm node

def _bn_world(C, dtype, with_res, Bs, gen, edge=None, centre_shift=0.0):
    """The joint batch (sum(Bs) maps of H x W, mask density 0.2-0.6 per map) and one MaskedBatchNorm per rank (equal, unless centre_shift moves
    rank 1's running mean by that many channel stds)."""
    from pillarnext_amd.models import MaskedBatchNorm

    n = sum(Bs)
    lo = [sum(Bs[:r]) for r in range(len(Bs))]
    dens = 0.2 + 0.4 * torch.rand((n, 1, 1, 1), device="cuda", generator=gen)
    mask = (torch.rand((n, 1, H, W), device="cuda", generator=gen) < dens).float()
    if edge in ("rank_none", "rank_one"):
        mask[lo[1]: lo[1] + Bs[1]] = 0
        if edge == "rank_one":
            mask[lo[1] + Bs[1] - 1, 0, H - 1, W - 3] = 1.0
    elif edge == "all_none":
        mask.zero_()
    ch_std = torch.rand(C, device="cuda", generator=gen) + 0.5
    ch_mean = (2 * torch.rand(C, device="cuda", generator=gen) - 1) * ch_std * 2.0
    x = _cl((torch.randn((n, C, H, W), device="cuda", generator=gen) * ch_std.view(1, -1, 1, 1) + ch_mean.view(1, -1, 1, 1)).to(dtype))
    res = _cl(torch.randn((n, C, H, W), device="cuda", generator=gen).to(dtype)) if with_res else None
    norm = MaskedBatchNorm(C, eps=EPS, momentum=MOM).cuda().train()
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, device="cuda", generator=gen) + 0.5)
        norm.bias.copy_(torch.randn(C, device="cuda", generator=gen) * 0.3)
        norm.running_mean.copy_(ch_mean + 0.1 * ch_std * torch.randn(C, device="cuda", generator=gen))
        norm.running_var.copy_(ch_std ** 2)
    norms = [copy.deepcopy(norm) for _ in Bs]
    if centre_shift:
        with torch.no_grad():
            norms[1].running_mean.add_(centre_shift * ch_std)
    return x, mask, res, norms, lo


def _bn_rank_fn(x, mask, res, norms, lo, Bs, relu, gy):
    from pillarnext_amd.models import masked_bn_act

    def fn(rank, token):
        sl = slice(lo[rank], lo[rank] + Bs[rank])
        n = copy.deepcopy(norms[rank])
        if token is not None:
            n.enable_sync(process_group=token)
        xa = _cl(x[sl].clone()).requires_grad_(True)
        ra = _cl(res[sl].clone()).requires_grad_(True) if res is not None else None
        y = masked_bn_act(xa, mask[sl].contiguous(), n, residual=ra, relu=relu)
        assert type(y.grad_fn).__name__ == "_MaskedBNActFnBackward"
        y.backward(_cl(gy[sl].clone()))
        return dict(y=y.detach(), dx=xa.grad, dres=None if ra is None else ra.grad, dgamma=n.weight.grad, dbeta=n.bias.grad, rm=n.running_mean,
                    rv=n.running_var, nbt=int(n.num_batches_tracked))
    return fn


def _bn_sync_check(tag, C, dtype, with_res, relu, Bs, gen, edge=None, centre_shift=0.0):
    x, mask, res, norms, lo = _bn_world(C, dtype, with_res, Bs, gen, edge, centre_shift)
    n0 = norms[0]
    # the batch statistics do not depend on the buffers: the joint statement is taken once; every rank's running statistics move from its own
    r = _bn_ref(x, mask, n0.weight.detach(), n0.bias.detach(), res, relu, n0.running_mean, n0.running_var, EPS, MOM)
    gy = torch.randn(x.shape, device="cuda", generator=gen)
    if relu:
        gy = gy * ((r["pre"].abs() > 2.0 ** -12 * r["prea"]) | (mask == 0))          # no ReLU gate within rounding of zero (_bn_check)
    gy = _cl(gy.to(dtype))
    rb = _bn_ref_backward(r, gy)
    rp = Replay(len(Bs))
    out = rp.run(_bn_rank_fn(x, mask, res, norms, lo, Bs, relu, gy))
    assert rp.passes == 3 and [tuple(k.shape) for k in rp.known] == [(2 * C + 1,), (2 * C,)], (rp.passes, [tuple(k.shape) for k in rp.known])
    assert float(rp.known[0][2 * C]) == float(mask.sum())                          # the count every rank divided by is the global one
    ulp = BF_OUT if dtype == torch.bfloat16 else 0.0
    xa = (r["x64"].abs() + r["mean"].abs().view(1, -1, 1, 1)) * r["invstd"].view(1, -1, 1, 1)
    sd, cnt = r["var"].sqrt(), r["cnt"]
    for k, o in enumerate(out):
        t = f"{tag} rank {k}/{len(Bs)}"
        sl = slice(lo[k], lo[k] + Bs[k])
        act = (mask[sl] != 0).expand_as(x[sl])
        assert bool((o["y"][~act] == 0).all()) and bool((o["dx"][~act] == 0).all()), (t, "inactive sites")
        if bool(act.any()):
            _check(t, "y", o["y"][act], r["y"][sl][act], (r["prea"] * r["m"])[sl][act], BN_REL, None, ulp)
            _check(t, "dx", o["dx"][act], rb["dx"][sl][act], rb["dxa"][sl][act], BN_REL, None, ulp)
        if res is not None:
            assert torch.equal(o["dres"].double(), rb["g"][sl]), (t, "dresidual is the gated upstream gradient, exactly")
        # parameter gradients: the LOCAL sums of the joint statement over this rank's samples (DistributedDataParallel averages them)
        g = rb["g"][sl]
        _check(t, "dgamma", o["dgamma"], (g * r["xhat"][sl]).sum(dim=(0, 2, 3)), (g.abs() * xa[sl]).sum(dim=(0, 2, 3)), BN_REL)
        _check(t, "dbeta", o["dbeta"], g.sum(dim=(0, 2, 3)), g.abs().sum(dim=(0, 2, 3)), BN_REL)
        # running statistics: the joint mean, the joint variance with the GLOBAL count, from this rank's old values
        rm0, rv0 = norms[k].running_mean.double(), norms[k].running_var.double()
        _check(t, "running_mean", o["rm"], (1 - MOM) * rm0 + MOM * r["mean"], rm0.abs() + MOM * (r["mean"].abs() + sd), BN_REL)
        _check(t, "running_var", o["rv"], (1 - MOM) * rv0 + MOM * r["var"] * cnt / (cnt - 1).clamp(min=1.0), rv0.abs() + MOM * r["var"] * 2, BN_REL)
        assert o["nbt"] == 1
    return out, r


@pytest.mark.parametrize("Bs", [[1, 2], [2, 1, 2]], ids=["world2", "world3"])
@pytest.mark.parametrize("with_res,relu", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [16, 64, 256])
def test_masked_bn_sync_equals_the_joint_batch(monkeypatch, C, dtype, with_res, relu, Bs):
    monkeypatch.setenv("PNX_MASKED_BN_HIP", "1")
    gen = torch.Generator(device="cuda").manual_seed(1000 + C + 2 * with_res + relu + 10 * (dtype == torch.bfloat16) + 100 * len(Bs))
    _bn_sync_check(f"masked BN sync C={C} {str(dtype)[6:]} res={with_res} relu={relu}", C, dtype, with_res, relu, Bs, gen)


@pytest.mark.parametrize("edge", ["rank_none", "rank_one", "all_none"])
def test_masked_bn_sync_edge_counts(monkeypatch, edge):
    """A rank with no active site (its sums are zero, its outputs zero, it still joins both collectives), a rank with exactly one (in the tail of
    the walks), no active site on any rank (the count clamps to 1, the mean is 0: the `none` case of
    test_masked_bn_edge_counts_match_the_torch_statement)."""
    monkeypatch.setenv("PNX_MASKED_BN_HIP", "1")
    Bs = [1, 2] if edge == "all_none" else [2, 1, 2]
    gen = torch.Generator(device="cuda").manual_seed(77)
    out, r = _bn_sync_check(f"masked BN sync edge {edge}", 64, torch.float32, True, True, Bs, gen, edge=edge)
    if edge == "all_none":
        assert float(r["cnt"]) == 1.0 and float(r["mean"].abs().max()) == 0.0
        for o in out:
            assert float(o["y"].abs().max()) == 0.0 and float(o["dx"].abs().max()) == 0.0 and float(o["dgamma"].abs().max()) == 0.0
    elif edge == "rank_none":
        o = out[1]
        assert float(o["y"].abs().max()) == 0.0 and float(o["dx"].abs().max()) == 0.0
        assert float(o["dgamma"].abs().max()) == 0.0 and float(o["dbeta"].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_masked_bn_sync_with_different_running_means(monkeypatch, dtype):
    """Rank 1's running mean is half a channel std away from rank 0's (no buffer broadcast: broadcast_buffers=False, a per-rank warm-up, a
    hand-rolled loop).  The node sums around the rank's running mean; batch statistics, y, dx and the gradients must still be those of the joint
    batch, at the same bars, and each rank's running mean moves from its own old value.  Before the sums were re-centred to 0 in front of the
    all-reduce (train_nodes._MaskedBNActFn._forward_hip) the ranks' sums were added as if they shared one centre, and the means were wrong by the
    shift times the other rank's share of the sites."""
    monkeypatch.setenv("PNX_MASKED_BN_HIP", "1")
    gen = torch.Generator(device="cuda").manual_seed(31 + (dtype == torch.bfloat16))
    _bn_sync_check(f"masked BN sync centres differ {str(dtype)[6:]}", 64, dtype, True, True, [1, 2], gen, centre_shift=0.5)


def test_masked_bn_without_sync_is_the_plain_launch_sequence(monkeypatch):
    """sync off: the node is stats -> reduce -> finalize AROUND THE RUNNING MEAN -> apply, bit for bit (restated here on the C entry points, with no
    collective replaced): the re-centring of the synchronised mode does not touch the single-rank arithmetic."""
    from pillarnext_amd import ops
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    monkeypatch.setenv("PNX_MASKED_BN_HIP", "1")
    C = 64
    gen = torch.Generator(device="cuda").manual_seed(5)
    x, mask, res, norms, lo = _bn_world(C, torch.float32, True, [2], gen)
    gy = _cl(torch.randn(x.shape, device="cuda", generator=gen))
    o = _bn_rank_fn(x, mask, res, norms, lo, [2], True, gy)(0, None)
    L = lib()
    n = copy.deepcopy(norms[0])
    nsite, nblk = x.shape[0] * H * W, int(L.pnx_masked_bn_blocks())
    mflat = mask.reshape(-1).contiguous()
    part = torch.empty((nblk, 2 * C + 1), dtype=torch.float32, device="cuda")
    check(L.pnx_masked_bn_stats(ptr(x), ops._DT[x.dtype], ptr(mflat), nsite, C, ptr(n.running_mean), ptr(part), stream_ptr()), "stats")
    s = torch.empty((2 * C + 1,), dtype=torch.float64, device="cuda")
    check(L.pnx_masked_bn_reduce(ptr(part), nblk, 2 * C + 1, ptr(s), stream_ptr()), "reduce")
    vec = torch.empty((4 * C + 1,), dtype=torch.float32, device="cuda")
    check(L.pnx_masked_bn_finalize(ptr(s), C, ptr(n.running_mean), ptr(n.weight), ptr(n.bias), float(n.eps), float(n.momentum), ptr(n.running_mean),
                                   ptr(n.running_var), ptr(n.num_batches_tracked), ptr(vec[:C]), ptr(vec[C:2 * C]), ptr(vec[2 * C:3 * C]),
                                   ptr(vec[3 * C:4 * C]), ptr(vec[4 * C:]), stream_ptr()), "finalize")
    y = torch.empty_like(x)
    check(L.pnx_masked_bn_apply(ptr(x), ptr(res), ops._DT[x.dtype], ptr(mflat), nsite, C, ptr(vec[2 * C:3 * C]), ptr(vec[3 * C:4 * C]), 1, ptr(y),
                                stream_ptr()), "apply")
    torch.cuda.synchronize()
    assert torch.equal(o["y"], y) and torch.equal(o["rm"], n.running_mean) and torch.equal(o["rv"], n.running_var)


# ---------------------------------------------------------------------------------------------------- fused training reader

PFN_TINY = 1e-300
# name: (frames per rank, points per frame (a rank's frames in order), seed -- picked on the CPU so that the joint case meets T.conditions' caps)
PFN_WORLDS = {
    "world2": ([1, 2], [[4_300], [5_600, 5_000]], 71),
    "world3_middle_out_of_range": ([1, 1, 1], [[5_200], [300], [4_700]], 72),       # every point of rank 1 outside the range: P = 0 there
    "world2_rank1_no_rows": ([1, 1], [[5_000], [0]], 73),                             # rank 1 holds a (0, 6) cloud
}


def _key(coords, shift=0):
    c = np.asarray(coords, np.int64)
    return ((c[:, 0] + shift) << 40) | (c[:, 1] << 20) | c[:, 2]


@functools.lru_cache(maxsize=None)
def pfn_world(name):
    """The clouds of every rank (frame indices 0 .. B_r - 1), the joint cloud (rank r's frames offset by the frames of the ranks before it) and the
    fp64 twin of ONE step on the joint cloud, computed once and shared, read-only.  Plain numpy: the conditions are asserted on the host."""
    Bs, counts, seed = PFN_WORLDS[name]
    rng = np.random.default_rng(seed)
    lo = [sum(Bs[:r]) for r in range(len(Bs))]
    clouds = []
    for r, per_frame in enumerate(counts):
        parts = [T._cloud(rng, n, T.G128, b) for b, n in enumerate(per_frame)]
        p = np.concatenate(parts) if parts else np.zeros((0, 6), np.float32)
        if name == "world3_middle_out_of_range" and r == 1:
            p[: len(p) // 2, 1] += 40.0
            p[len(p) // 2:, 2] -= 40.0
        clouds.append(np.ascontiguousarray(p[rng.permutation(len(p))], np.float32))
    joint = []
    for r, p in enumerate(clouds):
        q = p.copy()
        q[:, 0] += lo[r]
        joint.append(q)
    c = dict(name=name, pts=np.concatenate(joint), B=sum(Bs), geom=T.G128, F=5, prm=T.make_params(5, seed), gseed=seed + 500)
    s = T.step(c)
    c["ref"] = s
    frag, masked, positive = T.conditions(s)
    assert frag <= T.MAX_FRAGILE0 and masked <= T.MAX_MASKED1 and positive >= T.MIN_POSITIVE1, (name, frag, masked, positive)
    for a in (c["pts"], *clouds, *c["prm"].values(), *[x for x in s.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    order = np.argsort(_key(s["coords"]))
    return dict(c=c, Bs=Bs, lo=lo, clouds=clouds, order=order, keys=_key(s["coords"])[order])


def _joint_rows(w, coords, rank):
    """rows of the joint twin that hold the pillars `coords` of `rank`"""
    k = _key(coords, w["lo"][rank])
    pos = np.searchsorted(w["keys"], k)
    assert (pos < len(w["keys"])).all() and (w["keys"][np.minimum(pos, len(w["keys"]) - 1)] == k).all(), "a pillar the joint cloud does not have"
    return w["order"][pos]


def _pfn_rank_fn(w):
    c, s = w["c"], w["c"]["ref"]

    def fn(rank, token):
        net = make_net(c).enable_sync(process_group=token)
        fm, coords, _ = net(torch.from_numpy(np.array(w["clouds"][rank])).cuda(), w["Bs"][rank])
        assert type(fm.grad_fn).__name__ == "FusedPFNTrainBackward"
        co = coords.cpu().numpy()
        rows = _joint_rows(w, co, rank)
        fm.backward(torch.from_numpy(np.ascontiguousarray(s["G"][rows])).cuda().reshape(len(rows), 64))
        torch.cuda.synchronize()
        out = dict(feat_max=fm.detach(), coords=co, rows=rows)
        for i, pfn in enumerate(net.pfn_layers):
            out[f"dW{i}"], out[f"dgamma{i}"], out[f"dbeta{i}"] = pfn.linear.weight.grad, pfn.norm.weight.grad, pfn.norm.bias.grad
            out[f"rm{i}"], out[f"rv{i}"] = pfn.norm.running_mean, pfn.norm.running_var
            assert int(pfn.norm.num_batches_tracked) == 1
        return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    return fn


@pytest.mark.parametrize("name", list(PFN_WORLDS))
def test_fused_reader_sync_equals_the_joint_cloud(monkeypatch, name):
    """pfn_train.FusedPFNTrain with enable_sync(token) on every rank's cloud against pfn_train_ref on the joint cloud.  Per rank: coords are the
    joint pillars of the rank's frames and feat_max their rows, at the twin's feat_max_bar; the running statistics (momentum 1, zero buffers: the
    batch statistics, the variance times N'/(N' - 1) with the GLOBAL N') on every rank at the bars of test_gpu_pfn_train_vs_fp64.ratios.  The six
    parameter gradients are LOCAL sums: their sum over the ranks is held to the joint twin's bar plus U sum_r |got_r|, one fp32 rounding of each
    rank's stored gradient -- every term of the joint statement belongs to exactly one rank's rows and the statistics it is formed with are the
    global ones on every rank, so the ranks' errors add up to at most what one rank walking all rows is allowed."""
    monkeypatch.setenv("PNX_TRAIN_FUSED", "1")
    w = pfn_world(name)
    c, s, Bs, lo = w["c"], w["c"]["ref"], w["Bs"], w["lo"]
    rp = Replay(len(Bs))
    out = rp.run(_pfn_rank_fn(w))
    assert rp.passes == 5 and [tuple(k.shape) for k in rp.known] == [(65,), (128,), (128,), (64,)], (rp.passes, [tuple(k.shape) for k in rp.known])
    assert float(rp.known[0][64]) == s["N"]
    worst = {}

    def hold(k, err, bar):
        v = float((err / (bar + PFN_TINY)).max()) if err.size else 0.0
        worst[k] = max(worst.get(k, 0.0), v)

    seen = []
    for r, o in enumerate(out):
        jb = s["coords"][:, 0]
        mine = np.flatnonzero((jb >= lo[r]) & (jb < lo[r] + Bs[r]))
        assert np.array_equal(np.sort(o["rows"]), mine), (name, r, "coords are the joint pillars of the rank's frames")
        assert np.array_equal(o["coords"] + np.array([lo[r], 0, 0]), s["coords"][o["rows"]])
        assert o["feat_max"].shape == (len(mine), 64) and all(np.isfinite(o[k]).all() for k in o if k not in ("coords", "rows"))
        seen.append(o["rows"])
        hold("feat_max", np.abs(o["feat_max"] - s["feat_max"][o["rows"]]), s["feat_max_bar"][o["rows"]])
        for i in (0, 1):
            rm, rv, brm, brv = T.running(s[f"mu{i}"], s[f"var{i}"], s["N"], inp=s["stat1_in"] if i else (0.0, 0.0))
            hold(f"mean{i}", np.abs(o[f"rm{i}"] - rm), brm + T.U * np.abs(rm))
            hold(f"var{i}", np.abs(o[f"rv{i}"] - rv), brv + T.U * np.abs(rv))
        # what is exactly zero stays exactly zero on every rank: the closed channels, and the zero-gamma channel whose every maximum is 0
        assert (o["feat_max"][:, [5, 9]] == 0).all() and (o["dgamma1"][[5, 9]] == 0).all() and (o["dbeta1"][[5, 9]] == 0).all()
        assert (o["dW0"][7] == 0).all() and o["dgamma0"][7] == 0 and o["dbeta0"][7] == 0 and (o["dW1"][[5, 9]] == 0).all()
        if len(mine) == 0:
            assert all((o[k] == 0).all() for k in GRADS), (name, r, "a rank without a pillar has exactly-zero gradients")
    assert len(np.concatenate(seen)) == s["P"]
    for k in GRADS:
        tot = sum(o[k].astype(np.float64) for o in out)
        hold(k, np.abs(tot - s[k]), s[k + "_bar"] + T.U * sum(np.abs(o[k].astype(np.float64)) for o in out))
    frag, masked, positive = T.conditions(s)
    print(f"[pfn sync vs fp64] {name}: world {len(Bs)} N'={s['N']} P={s['P']} pillars per rank {[len(x) for x in seen]} fragile0 {100 * frag:.4f} % masked "
          f"{100 * masked:.2f} % positive {100 * positive:.0f} %  worst |err| / bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, (name, bad)

"""GPU: what runs BEHIND the convolutions of the timed inference step (csrc/decode.hip, k_sephead_lazy of csrc/sephead_lazy.h, the batched NMS of
csrc/iou3d.hip) at the shapes bench.py runs it at -- C2: head map 360 x 360, 12 frames, 6 tasks with 1+2+2+1+2+2 = 10 classes, pre_max 1000, post_max 83
(configs/pillarnext_b_nusc.yaml) -- against exact or fp64 statements of the same operation.

The small tests cannot reach, by construction: index bits >= 21 of the radix select's composites (every test there has fewer than 2^21 keys), the table walk
of k_rs_select (a list found in more than 256 chunk slots), a last lazy-head workgroup with fewer than kLzG rows, multi-class tasks at kernel level, 120
lists through one NMS launch.  Every case restates the launch's work split in Python, naming the constants of the .hip source it mirrors, and asserts that
its inputs reach the path it is there for; -rP prints the measured figures.

Bars.  Top-k and NMS: exact (one stable unsigned sort + cut; oracle.nms_rotated(..., "det") per list).  pnx_decode_keys: segment bits exact, validity exact
outside |score64 - threshold| <= 1e-6 (counted, at most 0.1 %), scores rtol 1e-5 (the decoder goldens' bar).  k_sephead_lazy, as in
tests/test_gpu_infer_kernels_at_scale.py: per element BF_REL x sum|terms| of the second convolution + one output rounding, plus one intermediate ulp x |w2|
for every intermediate whose fp64 value lies within BF_REL x sum|terms| of a rounding boundary (the kernel's fp32 sum may round that one the other way);
Frobenius error at most FRO_MARGIN x that of the once-rounded fp64 result; slots behind seg_len bit-zero; two calls bit-identical."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_infer_kernels_at_scale import FRO_MARGIN, OUT_ROUND  # noqa: E402  (the inference module's bars, unchanged)
from test_gpu_train_kernels_at_scale import BF_REL, TINY  # noqa: E402

# the C2 head: configs/pillarnext_b_nusc.yaml
B_C2, H_C2, W_C2 = 12, 360, 360
NCLS = [1, 2, 2, 1, 2, 2]
CLASS_TASK = [0, 1, 1, 2, 2, 3, 4, 4, 5, 5]
PRE_MAX, POST_MAX = 1000, 83
# csrc/decode.hip
kRsBins, kRsSlots, kRsChunk = 2048, 4, 16384
RS_SHIFT = [53, 42, 32, 21, 10, 0]          # rs_shift(p)
# csrc/conv3x3.hip
kLzG = 32
SIGN = -0x8000000000000000


# ---------------------------------------------------------------------------------------------------- segmented top-k (pnx_decode_topk)

def _blocked_segments(g, B, HW, ncls):
    """key i = t * B * HW + b * HW + cell (pnx_decode_keys per task, concatenated): list = b * nc_total + cls_off[t] + label"""
    nct, parts, off = sum(ncls), [], 0
    for nc in ncls:
        b = torch.arange(B, device="cuda").repeat_interleave(HW)
        parts.append(b * nct + off + torch.randint(0, nc, (B * HW,), device="cuda", generator=g))
        off += nc
    return torch.cat(parts)


def _topk_case(layout):
    g = torch.Generator(device="cuda").manual_seed(21)
    HW = H_C2 * W_C2
    if layout == "mixed":                                                   # few lists over many chunks: the table walk of k_rs_select
        S, n = 4, 4_500_000
        seg = torch.randint(0, 3, (n,), device="cuda", generator=g)
        sc = (torch.rand((n,), device="cuda", generator=g) * 0.9 + 0.1).to(torch.bfloat16).float()
        valid = torch.rand((n,), device="cuda", generator=g) < 0.08
        # list 3: 999 keys of score 0.9, then two keys of score 0.5 whose indices differ in bit 21 ONLY, then lower scores
        idx = torch.randperm(n, device="cuda", generator=g)[:1400]
        x = 1_000_003
        idx = idx[(idx != x) & (idx != x + (1 << 21))]
        seg[idx], valid[idx] = 3, True
        sc[idx[:999]], sc[idx[999:]] = 0.9, 0.25
        for i in (x, x + (1 << 21)):
            seg[i], valid[i], sc[i] = 3, True, 0.5
        special = dict(tie=3)
    else:
        S, n = B_C2 * sum(NCLS), len(NCLS) * B_C2 * HW
        seg = _blocked_segments(g, B_C2, HW, NCLS)
        if layout == "all_equal":
            sc = torch.full((n,), 0.25, device="cuda")
            valid = torch.ones((n,), dtype=torch.bool, device="cuda")
        else:
            sc = (torch.rand((n,), device="cuda", generator=g) * 0.9 + 0.1).to(torch.bfloat16).float()
            valid = torch.rand((n,), device="cuda", generator=g) < 0.08
        # the keys of list (sample 4, class 1) -- task 1 -- straddle index 2^21: ONE score in that list, so that the pre_max-th and the next key tie
        # in score; thinned so that exactly pre_max valid keys lie below 2^21
        tie = 4 * sum(NCLS) + 1
        mine = (seg == tie).nonzero().flatten()
        assert int(mine[0]) < (1 << 21) < int(mine[-1])
        sc[mine], valid[mine] = 0.5, True
        below = mine[mine < (1 << 21)]
        valid[below[: below.numel() - PRE_MAX]] = False
        empty, few = 7 * sum(NCLS) + 3, 9 * sum(NCLS) + 8
        valid[seg == empty] = False
        fk = (seg == few).nonzero().flatten()
        valid[fk[40:]] = False
        special = dict(tie=tie, empty=empty, few=few)
    low = 0xFFFFFFFF - sc.view(torch.int32).to(torch.int64)
    keys = torch.where(valid, (seg.to(torch.int64) << 32) | low, torch.full_like(low, -1))
    return keys, S, special


@pytest.mark.parametrize("layout", ["blocked", "all_equal", "mixed"])
def test_topk_at_benchmark_scale_equals_the_stable_sort(layout):
    """pnx_decode_topk at 9 331 200 keys / 120 lists / pre_max 1000 (and, "mixed", 4 lists over 275 chunks) == one stable unsigned sort + cut: keys, order,
    seg_len, seg_total, seg_start; the call repeated through the same workspace.  Exact."""
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    L = lib()
    keys, S, special = _topk_case(layout)
    n, k = keys.numel(), PRE_MAX
    # ---- reference
    skeys, order = torch.sort(keys ^ SIGN, stable=True)
    bounds = (torch.arange(S + 1, device="cuda", dtype=torch.int64) << 32) ^ SIGN
    st = torch.searchsorted(skeys, bounds)
    skeys = skeys ^ SIGN
    tot = st[1:] - st[:-1]
    ln = torch.clamp(tot, max=k)
    jj = torch.arange(k, device="cuda")
    sel = jj[None, :] < ln[:, None]                                           # (S, k)
    pos = (st[:S, None] + jj[None, :]).clamp(max=n - 1)
    want_o, want_k = order[pos][sel], skeys[pos][sel]
    # ---- the work split (csrc/decode.hip: k_rs_hist one workgroup per kRsChunk keys with kRsSlots LDS histograms; k_rs_select's s_list holds 256 slots)
    nchunks = -(-n // kRsChunk)
    valid = keys != -1
    ck = torch.arange(n, device="cuda") // kRsChunk
    pairs = torch.unique(ck[valid] * S + (keys[valid] >> 32))                 # (chunk, list) pairs that hold a valid key
    pairs = torch.stack([pairs // S, pairs % S])
    per_chunk = torch.bincount(pairs[0], minlength=nchunks)
    slots_of_list = torch.bincount(pairs[1][per_chunk[pairs[0]] <= kRsSlots], minlength=S)   # a chunk with <= kRsSlots lists gives each a slot
    hi_bits = int((want_o >> RS_SHIFT[3]).max())
    print(f"topk[{layout}]: {n} keys, {S} lists, {nchunks} chunks x {kRsSlots} slots = {nchunks * kRsSlots}; lists per chunk <= {int(per_chunk.max())}; "
          f"most slots of one list {int(slots_of_list.max())}; highest index digit of pass 3 among the selected keys {hi_bits}; "
          f"lists cut at pre_max {int((tot > k).sum())}, short {int(((tot < k) & (tot > 0)).sum())}, empty {int((tot == 0).sum())}")
    assert int(sel.sum()) > 0
    if layout == "mixed":
        assert int(slots_of_list.max()) > 256, "no list is found in more than 256 chunk slots: the table walk does not run"
        assert int(per_chunk.max()) <= kRsSlots
    else:
        assert n == 9_331_200 and S == 120
        assert hi_bits >= 4, "no selected key above 2^23"
        lo = torch.full((S,), n, device="cuda", dtype=torch.int64).scatter_reduce(0, sel.nonzero()[:, 0], want_o, "amin")
        assert int(((lo >= (1 << 21)) & (ln == k)).sum()) > 0 and int(((lo >= (1 << 23)) & (ln == k)).sum()) > 0, "no full list wholly above 2^21 / 2^23"
        assert int(tot[special["empty"]]) == 0 and 0 < int(tot[special["few"]]) <= 40
    assert hi_bits >= 1, "index bit 21 is zero in every selected key"
    s = special["tie"]
    a0 = int(st[s])
    assert int(tot[s]) > k and int(skeys[a0 + k - 1]) == int(skeys[a0 + k]), "the pre_max-th and the next key of the tie list do not tie in score"
    diff = int(order[a0 + k - 1]) ^ int(order[a0 + k])
    assert diff >> 21 != 0 and (layout != "mixed" or diff == 1 << 21), hex(diff)
    # ---- the kernel, twice through one workspace
    out_k = torch.empty((S * k,), dtype=torch.int64, device="cuda")
    out_o = torch.empty((S * k,), dtype=torch.int64, device="cuda")
    out_s = torch.empty((S,), dtype=torch.int64, device="cuda")
    out_l = torch.empty((S,), dtype=torch.int32, device="cuda")
    out_t = torch.empty((S,), dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.pnx_decode_topk_workspace_bytes(n, S)) + 256, dtype=torch.uint8, device="cuda")
    for rep in range(2):
        out_k.fill_(-7), out_o.fill_(-7)
        check(L.pnx_decode_topk(ptr(keys), n, S, k, ptr(out_k), ptr(out_o), ptr(out_s), ptr(out_l), ptr(out_t), ptr(ws), ws.numel(), stream_ptr()),
              "pnx_decode_topk")
        assert torch.equal(out_t.long(), tot), (rep, "seg_total", (out_t.long() != tot).nonzero().flatten()[:8].tolist())
        assert torch.equal(out_l.long(), ln), (rep, "seg_len", (out_l.long() != ln).nonzero().flatten()[:8].tolist())
        assert torch.equal(out_s, torch.arange(S, device="cuda") * k), (rep, "seg_start")
        bad_o = (out_o.view(S, k)[sel] != want_o)
        bad_k = (out_k.view(S, k)[sel] != want_k)
        lists = sel.nonzero()[:, 0]
        assert not bool(bad_o.any()), (rep, "order differs in lists", torch.unique(lists[bad_o])[:8].tolist(), int(bad_o.sum()))
        assert not bool(bad_k.any()), (rep, "keys differ in lists", torch.unique(lists[bad_k])[:8].tolist(), int(bad_k.sum()))


# ---------------------------------------------------------------------------------------------------- score keys (pnx_decode_keys)

def _f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize("dtype,has_iou,ncls", [("bfloat16", True, 2), ("bfloat16", False, 1), ("float16", True, 1), ("float16", False, 2)])
def test_decode_keys_on_the_full_map_against_fp64(dtype, has_iou, ncls):
    """k_decode_keys (lazy packing: [iou] hm in 16 channels) on the 12 x 360 x 360 map against centerhead.py:259,341-354 in fp64: sigmoid, first maximal class,
    score > threshold, clamp((iou + 1) / 2, 0, 1), score^(1 - a) * iou^a."""
    from pillarnext_amd._lib import PNX_BF16, PNX_F16, check, lib, ptr, stream_ptr
    from pillarnext_amd.decode import pack_task

    dt = getattr(torch, dtype)
    B, H, W, C, nct, cls_off, thr = B_C2, H_C2, W_C2, 16, sum(NCLS), 3, 0.1
    rect = [0.68, 0.2][:ncls]
    g = torch.Generator(device="cuda").manual_seed(31 + ncls)
    x = torch.randn((B, H, W, C), device="cuda", generator=g)
    x[..., int(has_iou):] = x[..., int(has_iou):] * 1.5 - 2.19            # class logits around the head's initial bias
    if has_iou:
        x[..., 0] = x[..., 0] * 0.8                                         # (iou + 1) / 2 leaves [0, 1] on both sides
    x = x.to(dt)
    xm = x.permute(0, 3, 1, 2)                                              # (B, 16, H, W) channels_last
    assert xm.is_contiguous(memory_format=torch.channels_last)
    desc = pack_task(C, has_iou, ncls, cls_off, H, W, 4, (0.075, 0.075), (-54.0, -54.0), thr, [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], rect, lazy=True)
    n = B * H * W
    nb = -(-n // 256)                                                       # pnx_decode_keys: one thread per cell, 256 per workgroup
    print(f"decode_keys[{dtype}, iou {has_iou}, {ncls} classes]: {n} cells on {nb} workgroups of 256")
    keys = torch.empty((n,), dtype=torch.int64, device="cuda")
    check(lib().pnx_decode_keys(ptr(xm), PNX_BF16 if dt == torch.bfloat16 else PNX_F16, B, nct, desc, ptr(keys), stream_ptr()), "pnx_decode_keys")
    # ---- fp64
    o = int(has_iou)
    p = torch.sigmoid(x[..., o:o + ncls].double().reshape(n, ncls))
    best, lab = p[:, 0].clone(), torch.zeros((n,), dtype=torch.int64, device="cuda")
    for c in range(1, ncls):                                                # the FIRST maximal class (torch.max)
        up_ = p[:, c] > best
        best, lab = torch.where(up_, p[:, c], best), torch.where(up_, torch.full_like(lab, c), lab)
    ok = best > _f32(thr)
    a = torch.tensor([_f32(r) for r in rect], dtype=torch.float64, device="cuda")[lab]
    sc = best ** (1.0 - a)
    if has_iou:
        sc = sc * torch.clamp((x[..., 0].double().reshape(n) + 1.0) * 0.5, 0.0, 1.0) ** a
    b = torch.arange(n, device="cuda") // (H * W)
    seg = b * nct + cls_off + lab
    # ---- compare
    got_ok = keys != -1
    border = (best - _f32(thr)).abs() <= 1e-6
    nbord = int(border.sum())
    print(f"  valid {int(ok.sum())} of {n}; cells within 1e-6 of the threshold: {nbord} (left out of the validity check)")
    assert nbord <= 1e-3 * n and int(ok.sum()) > n // 10 and int((~ok).sum()) > n // 10
    assert torch.equal(got_ok[~border], ok[~border])
    both = got_ok & ok
    assert torch.equal((keys >> 32)[both], seg[both]), "segment bits"
    if ncls > 1:
        assert int((lab[both] == 1).sum()) > n // 50
    got_sc = (0xFFFFFFFF - (keys & 0xFFFFFFFF)).to(torch.int32).view(torch.float32)[both]
    want = sc[both]
    rel = ((got_sc.double() - want).abs() / want.abs().clamp(min=1e-30)).max().item()
    ulp = (got_sc.view(torch.int32).long() - want.float().view(torch.int32).long()).abs().max().item()
    print(f"  scores: worst relative error {rel:.3e} (bar 1e-5, ratio {rel / 1e-5:.3f}), worst distance to the rounded fp64 score {ulp} ulp")
    assert bool(((got_sc.double() - want).abs() <= 1e-5 * want.abs()).all())
    if has_iou:
        assert int((sc[both] == 0).sum()) > 0, "no iou clamped to 0"


# ---------------------------------------------------------------------------------------------------- lazy SepHead (k_sephead_lazy)

OFF, K = [0, 2, 3, 6, 8], [2, 1, 3, 2, 2]      # outputs of the five regression branches: reg 2 | height 1 | dim 3 | rot 2 | vel 2


def _lazy_weights(seed, dt):
    g = torch.Generator().manual_seed(seed)
    W1 = (torch.randn((320, 64, 3, 3), generator=g) * 0.06).to(dt).float()
    b1 = torch.randn((320,), generator=g) * 0.1
    W2 = torch.zeros((10, 320, 3, 3))
    for j in range(5):
        W2[OFF[j]:OFF[j] + K[j], 64 * j:64 * (j + 1)] = torch.randn((K[j], 64, 3, 3), generator=g) * 0.06
    W2 = W2.to(dt).float()
    b2 = torch.randn((10,), generator=g) * 0.1
    return W1.cuda(), b1.cuda(), W2.cuda(), b2.cuda()


def _w2m(W2):
    m = torch.zeros((9 * 320, 10), device=W2.device)
    for pos in range(9):
        m[pos * 320:(pos + 1) * 320] = W2[:, :, pos // 3, pos % 3].t()
    return m


def _ulp(r, dt):
    """spacing of the storage type at the (already rounded) fp64 value r, and whether |r| is a power of two (the spacing below it is half of that)"""
    e = torch.floor(torch.log2(r.abs().clamp(min=1e-300)))
    e = e.clamp(min=-126.0 if dt == torch.bfloat16 else -14.0)
    return torch.pow(2.0, e - (7 if dt == torch.bfloat16 else 10)), r.abs() == torch.pow(2.0, e)


def _lazy_ref(up, W1, b1, W2, b2, lc, dt, chunk=4096):
    """fp64 at the candidate cells lc = b * H * W + cell: conv 1 + bias, ReLU, rounded to dt (zero outside the map), conv 2 + bias; returns the fp64 value
    before the output rounding, sum|terms| of conv 2 and the allowance for intermediates that sit on a rounding boundary"""
    Bn, _, H, W = up.shape
    upn = up.permute(0, 2, 3, 1)                                            # (B, H, W, 64) view of the channels_last map
    w1 = W1.double().permute(2, 3, 1, 0).reshape(576, 320)                  # rows (ky, kx, cin)
    w2 = torch.stack([W2[:, :, p // 3, p % 3].double().t() for p in range(9)])   # (pos, 320, 10)
    d5 = torch.arange(5, device=lc.device) - 2
    d3 = torch.arange(3, device=lc.device)
    ref, mag, flip = [], [], []
    for c0 in range(0, lc.numel(), chunk):
        l = lc[c0:c0 + chunk]
        b, y, x = l // (H * W), (l % (H * W)) // W, l % W
        yy, xx = y[:, None] + d5[None, :], x[:, None] + d5[None, :]          # (N, 5)
        iny, inx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
        patch = upn[b[:, None, None], yy.clamp(0, H - 1)[:, :, None], xx.clamp(0, W - 1)[:, None, :]].double()       # (N, 5, 5, 64)
        patch = patch * (iny[:, :, None] & inx[:, None, :])[..., None]
        N = l.numel()
        # the nine neighbour positions' 3 x 3 windows: (N, 9, 3, 3, 64)
        wy = (d3[:, None] + d3[None, :])                                     # window row index [pos row][tap row]
        cols = patch[:, wy[:, None, :, None], wy[None, :, None, :]]          # (N, 3, 3, 3, 3, 64): [py][px][ky][kx]
        cols = cols.reshape(N * 9, 576)
        pre = cols @ w1 + b1.double()
        s1 = cols.abs() @ w1.abs() + b1.double().abs()
        t = torch.relu(pre)
        r = t.float().to(dt).double()
        u, pow2 = _ulp(r, dt)
        tol1 = BF_REL * s1 + TINY
        half = torch.where(pow2 & (t < r), 0.25 * u, 0.5 * u)               # distance from r to the rounding boundary on t's side
        near = ((half - (t - r).abs()) <= tol1) | (pre.abs() <= tol1)       # ... or the ReLU's kink
        inside = (iny[:, 1:4, None] & inx[:, None, 1:4]).reshape(N * 9, 1)  # neighbour position inside the map
        r, slack = r * inside, torch.where(near, u + tol1, torch.zeros_like(u)) * inside
        r, slack = r.view(N, 9, 320), slack.view(N, 9, 320)
        ref.append(torch.einsum("npc,pco->no", r, w2) + b2.double())
        mag.append(torch.einsum("npc,pco->no", r.abs(), w2.abs()) + b2.double().abs())
        flip.append(torch.einsum("npc,pco->no", slack, w2.abs()))
    return torch.cat(ref), torch.cat(mag), torch.cat(flip)


def _lazy_case(dt, B, H, W, class_task, lens_cycle, seed, every):
    from pillarnext_amd import ops

    nc, T = len(class_task), max(class_task) + 1
    S, HW = B * nc, H * W
    g = torch.Generator(device="cuda").manual_seed(seed)
    tasks, raw = [], []
    for ti in range(T):
        W1, b1, W2, b2 = _lazy_weights(100 + seed + ti, dt)
        up = torch.randn((B, H, W, 64), device="cuda", generator=g).to(dt).permute(0, 3, 1, 2)
        assert up.is_contiguous(memory_format=torch.channels_last)
        raw.append((up, W1, b1, W2, b2))
        tasks.append((up, ops.conv3x3_pack_weights(W1, dtype=dt), b1, ops.sephead_lazy_pack_w2(_w2m(W2)), b2))
    lens = [lens_cycle[(7 * s + s // nc) % len(lens_cycle)] for s in range(S)]
    seg_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    local = torch.randint(0, B * HW, (S, PRE_MAX), device="cuda", generator=g)
    corners = torch.tensor([0, W - 1, (H - 1) * W, HW - 1, W // 2, (H - 1) * W + 5, 7 * W, 8 * W - 1], device="cuda")   # corners, both edges of both axes
    smp = torch.arange(B, device="cuda")
    local[:, :8] = corners[None, :] + (torch.arange(S, device="cuda")[:, None] % B) * HW
    local[:, 8:8 + B] = smp[None, :] * HW + torch.randint(0, HW, (S, B), device="cuda", generator=g)     # every sample index in every full list
    local[:, 40:48] = local[:, 0:8]                                                                       # duplicates, in another workgroup
    local[:, PRE_MAX - 4:] = local[:, 3:4] + 0                                                            # corners in the last, partial workgroup
    # ---- work split: pnx_sephead_lazy launches batch * nc_total * bps workgroups of kLzG candidates, bps = ceil(pre_max / kLzG)
    bps = -(-PRE_MAX // kLzG)
    last_rows = PRE_MAX - (bps - 1) * kLzG
    nfull = sum(1 for v in lens if v > (bps - 1) * kLzG)
    print(f"sephead_lazy[{dt}]: {S} lists x {PRE_MAX} -> {S * bps} workgroups of {kLzG} candidates, {bps} per list, the last with {last_rows} rows "
          f"({nfull} lists reach it); {T} tasks, class map {class_task}; {sum(lens)} candidates; lengths {sorted(set(lens))}")
    assert last_rows < kLzG and nfull > 0
    if dt == torch.bfloat16:
        assert S * bps == 3840
    got = ops.sephead_lazy(tasks, class_task, B, local, seg_len, PRE_MAX)
    again = ops.sephead_lazy(tasks, class_task, B, local, seg_len, PRE_MAX)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ"
    valid = torch.arange(PRE_MAX, device="cuda")[None, :] < seg_len[:, None]
    assert bool((got.view(torch.int32)[~valid] == 0).all()), "slots behind seg_len are not bit-zero"
    assert {int(v) for v in torch.unique(local[valid] // HW).tolist()} == set(range(B))
    # ---- fp64 at the candidates of the checked lists: every `every`-th list plus the first list of each length and of each class
    pick = set(range(0, S, every))
    for v in set(lens):
        pick.add(lens.index(v))
    for c in range(nc):
        pick.add(next(s for s in range(c, S, nc) if lens[s] == PRE_MAX))
    worst, fro_g, fro_r, ncmp, nflip = 0.0, 0.0, 0.0, 0, 0
    for ti in range(T):
        ls = [s for s in sorted(pick) if class_task[s % nc] == ti and lens[s] > 0]
        if not ls:
            continue
        idx = torch.tensor(ls, device="cuda")
        v = valid[idx]
        lc = local[idx][v]
        up, W1, b1, W2, b2 = raw[ti]
        ref, mag, flip = _lazy_ref(up, W1, b1, W2, b2, lc, dt)
        g_ = got[idx][v].double()
        once = ref.float().to(dt).double()
        bar = BF_REL * mag + OUT_ROUND[dt] * ref.abs() + flip + TINY
        err = (g_ - ref).abs()
        worst = max(worst, float((err / bar).max()))
        bad = err > bar
        assert not bool(bad.any()), (ti, int(bad.sum()), float((err / bar).max()), bad.nonzero()[:4].tolist())
        fro_g += float(((g_ - ref) ** 2).sum())
        fro_r += float(((once - ref) ** 2).sum())
        ncmp += ref.numel()
        nflip += int((flip > 0).sum())
        assert float(ref.abs().mean()) > 0.05
    assert ncmp > 0
    ratio = (fro_g / fro_r) ** 0.5
    print(f"  compared {ncmp} outputs of {len(pick)} lists in fp64: worst error / bar {worst:.3f}; Frobenius error / once-rounded reference {ratio:.4f} "
          f"(bar {FRO_MARGIN}); outputs with a boundary allowance {nflip}")
    assert ratio <= FRO_MARGIN, ratio


def test_lazy_sephead_at_the_c2_shape_against_fp64():
    """bf16, the benchmark's six tasks and class map, 12 frames of 360 x 360, 120 lists x 1000."""
    _lazy_case(torch.bfloat16, B_C2, H_C2, W_C2, CLASS_TASK, [1000, 0, 1, 31, 32, 33, 257, 1000, 640, 999, 1000], seed=5, every=7)


def test_lazy_sephead_f16_at_the_waymo_map_size_against_fp64():
    """f16 (C5: 1504 / 4 = 376 cells a side), three one-class tasks."""
    _lazy_case(torch.float16, 4, 376, 376, [0, 1, 2], [1000, 0, 1, 31, 32, 33, 300, 1000], seed=9, every=3)


# ---------------------------------------------------------------------------------------------------- batched rotated NMS

def _cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def test_batched_nms_at_120_segments_vs_oracle(oracle):
    """120 lists at stride pre_max = 1000 in ONE launch, seg_len mixed, per-class thresholds, the workspace sized as launch_lazy_fused sizes it
    (pnx_nms_workspace_bytes(S * pre_max, S, pre_max)): keep lists and counts bit-exact against oracle.nms_rotated(..., "det"); post_max = 83 a prefix."""
    from pillarnext_amd import synth
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    L = lib()
    S, k = B_C2 * sum(NCLS), PRE_MAX
    cyc = [1000, 0, 1, 63, 64, 65, 1000, 517, 999, 257, 256]
    lens = [cyc[(7 * s + s // 10) % len(cyc)] for s in range(S)]
    thr_cls = [0.2, 0.2, 0.25, 0.2, 0.7, 0.1, 0.2, 0.55, 0.2, 0.2]
    thr = np.asarray([thr_cls[s % 10] for s in range(S)], np.float32)
    boxes = np.zeros((S * k, 7), np.float32)
    segs = []
    for s in range(S):
        b = synth.clustered_boxes(k, 900 + s)[0]                              # the slots behind seg_len hold boxes too: they must not take part
        boxes[s * k:(s + 1) * k] = b
        segs.append(b[:lens[s]])
    cb = -(-k // 64)
    print(f"nms: {S} segments x up to {k} boxes, {cb} mask words per box, {S * cb * (cb + 1) // 2} tiles; lengths {sorted(set(lens))}")
    d_boxes, d_off = _cu(boxes), _cu(np.arange(S + 1) * k, torch.int32)
    d_len, d_thr = _cu(np.asarray(lens), torch.int32), _cu(thr)
    ws = torch.empty(max(int(L.pnx_nms_workspace_bytes(S * k, S, k)), 1), dtype=torch.uint8, device="cuda")
    res = {}
    for post in (0, POST_MAX):
        keep = torch.full((S * k,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        check(L.pnx_nms_rotated_batched(ptr(d_boxes), ptr(d_off), ptr(d_len), S, k, ptr(d_thr), post, ptr(keep), ptr(cnt), ptr(ws), ws.numel(), stream_ptr()),
              "pnx_nms_rotated_batched")
        res[post] = (keep.cpu().numpy().reshape(S, k), cnt.cpu().numpy())
    # the candidate-pair list, for the record only (printed, nothing is asserted on it).  This restates csrc/iou3d.hip nms_layout: pair_cap = min(S * cb * 64 *
    # 32, 2^24), counts_off = mask_off - 256, counts[0] = pairs appended; if that layout changes, change these three lines with it
    pair_cap = min(S * cb * 64 * 32, 1 << 24)
    mask_off = int(L.pnx_nms_workspace_bytes(1, S, k)) - cb * 8 - 8
    appended = int(ws[mask_off - 256: mask_off - 252].view(torch.int32)[0])
    print(f"  candidate pairs appended {appended} of capacity {pair_cap}: the pair list {'overflowed' if appended > pair_cap else 'did not overflow'}")
    keep0, cnt0 = res[0]
    keep83, cnt83 = res[POST_MAX]
    checked = sorted(set(range(0, S, 7)) | {lens.index(v) for v in set(lens)})   # the oracle is O(n^2) on the host: every 7th list and one of each length
    nsup = 0
    for s in range(S):
        assert cnt83[s] == min(cnt0[s], POST_MAX), s
        assert np.array_equal(keep83[s, :cnt83[s]], keep0[s, :cnt83[s]]), s
        assert cnt0[s] <= lens[s]
        if s in checked:
            ref = oracle.nms_rotated(segs[s], float(thr[s]), "det") if lens[s] else np.zeros(0, np.int64)
            assert cnt0[s] == len(ref), (s, cnt0[s], len(ref))
            assert np.array_equal(keep0[s, :cnt0[s]], ref), s
            nsup += lens[s] - len(ref)
    det = oracle.boxes_iou_bev(segs[0][:300], segs[0][:300], "det")
    print(f"  {len(checked)} lists against the oracle, {nsup} boxes suppressed in them; IoU > 0 in {float((det > 0).mean()):.3f} of the pairs of list 0")
    assert nsup > 0 and (det > 0).mean() > 0.01


def test_nms_refuses_a_workspace_without_room_for_the_mask_words():
    """pnx_nms_rotated_batched must check the mask words behind its layout, not only the layout: declaring fewer bytes than
    pnx_nms_workspace_bytes(1, S, max_seg_len) -- the smallest size of any call with a box in it -- is PNX_ERR_WORKSPACE.  The buffer really has the full
    size, so the call cannot write out of bounds whichever way the check goes."""
    from pillarnext_amd import synth
    from pillarnext_amd._lib import lib, ptr, stream_ptr

    L = lib()
    S, k = 3, 1000
    boxes = _cu(np.concatenate([synth.clustered_boxes(k, 50 + s)[0] for s in range(S)]))
    off, thr = _cu(np.arange(S + 1) * k, torch.int32), _cu(np.full(S, 0.2, np.float32))
    keep = torch.empty((S * k,), dtype=torch.int32, device="cuda")
    cnt = torch.empty((S,), dtype=torch.int32, device="cuda")
    full = int(L.pnx_nms_workspace_bytes(S * k, S, k))
    one = int(L.pnx_nms_workspace_bytes(1, S, k))
    cb = -(-k // 64)
    mask_off = one - cb * 8 - 8
    assert full == mask_off + S * k * cb * 8 + 8
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    call = lambda nbytes: L.pnx_nms_rotated_batched(ptr(boxes), ptr(off), None, S, k, ptr(thr), 0, ptr(keep), ptr(cnt), ptr(ws), ctypes.c_size_t(nbytes),  # noqa: E731
                                                    stream_ptr())
    PNX_ERR_WORKSPACE = -3                                                   # include/pnx.h
    for nbytes in (mask_off, mask_off + 16, one - 8):                        # the layout alone; two mask words; one word short of one box's row
        assert call(nbytes) == PNX_ERR_WORKSPACE, nbytes
    assert call(one) == 0 and call(full) == 0
    torch.cuda.synchronize()
    assert int(cnt.min()) > 0


# ---------------------------------------------------------------------------------------------------- candidate boxes (pnx_decode_boxes_lazy)

VS, PCR, OSF = (0.075, 0.075), (-54.0, -54.0), 4
kDecodeThreads = 256                                                         # csrc/decode.hip: k_decode_boxes_lazy, one workgroup per list


def _descs(lim, has_iou=True, thr=0.1):
    from pillarnext_amd.decode import pack_task

    out, off = [], 0
    for nc in NCLS:
        out.append(pack_task(16, has_iou, nc, off, H_C2, W_C2, OSF, VS, PCR, thr, lim, [0.5, 0.5][:nc], lazy=True))
        off += nc
    return out


def test_decode_boxes_lazy_at_lists_of_1000():
    """k_decode_boxes_lazy on 120 lists of 1000 / 999 / 257 / 256 / 1 / 0 candidates with a post_center_limit_range that cuts a known share: survivors and their
    order exact, seg_len exact, the flag exactly any(lost a candidate and seg_total > pre_max) in three calls (cut lists lose nothing; one cut list loses; no list
    is cut), scores bit-equal to the key's, boxes against fp64 within the decoder golden's 1e-4.  The range decision is taken in fp64; candidates whose centre
    lies within 1e-5 of a limit are counted (cap 0.1 %) -- the inputs are built so that there is none."""
    from pillarnext_amd._lib import check, lib, ptr, stream_ptr

    L = lib()
    S, k, HW, nct = B_C2 * sum(NCLS), PRE_MAX, H_C2 * W_C2, sum(NCLS)
    lim = [-40.0, -40.0, -1.0, 40.0, 40.0, 1.0]
    g = torch.Generator(device="cuda").manual_seed(41)
    cyc = [1000, 999, 257, 256, 1, 0, 1000]
    lens = [1000 if s % nct == 0 else cyc[(3 * s + s // nct) % len(cyc)] for s in range(S)]
    steps = -(-max(lens) // kDecodeThreads)
    print(f"decode_boxes_lazy: {S} workgroups of {kDecodeThreads}; a list of {max(lens)} takes {steps} compaction steps; lengths {sorted(set(lens))}")
    assert steps == 4 and {1000, 999, 257, 256, 1, 0} <= set(lens)
    seg_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    cell = torch.randint(0, HW, (S, k), device="cuda", generator=g)
    central = (torch.arange(S, device="cuda") % nct == 0)                    # the lists of class 0: candidates from the middle of the map only
    cc = torch.randint(150, 210, (S, k, 2), device="cuda", generator=g)
    cell = torch.where(central[:, None], cc[..., 0] * W_C2 + cc[..., 1], cell)
    smp = torch.arange(S, device="cuda") // nct
    koff = torch.tensor([t * B_C2 * HW for t in range(len(NCLS) + 1)], dtype=torch.int64, device="cuda")
    task = torch.tensor([CLASS_TASK[s % nct] for s in range(S)], device="cuda")
    order = (koff[task][:, None] + smp[:, None] * HW + cell).reshape(-1).contiguous()
    sc = torch.sort(torch.rand((S, k), device="cuda", generator=g) * 0.9 + 0.1, dim=1, descending=True)[0]
    skeys = ((torch.arange(S, device="cuda")[:, None] << 32) | (0xFFFFFFFF - sc.view(torch.int32).to(torch.int64))).reshape(-1).contiguous()
    seg_start = (torch.arange(S, device="cuda", dtype=torch.int64) * k).contiguous()
    cand = torch.randn((S, k, 10), device="cuda", generator=g)
    cand[..., 0:2] = torch.rand((S, k, 2), device="cuda", generator=g)
    cand[..., 2] = torch.where(central[:, None], torch.zeros_like(cand[..., 2]), cand[..., 2] * 0.5)
    cand[..., 3:6] *= 0.4
    cand = cand.to(torch.bfloat16).float()                                   # what k_sephead_lazy writes: bf16 values in fp32
    # ---- fp64 (centerhead.py:285-303, 343-346); the constants as the fp32 descriptor holds them
    f32 = lambda v: float(np.float32(v))  # noqa: E731

    def centres(c):
        x = ((cell % W_C2).double() + c[..., 0].double()) * OSF * f32(VS[0]) + f32(PCR[0])
        y = ((cell // W_C2).double() + c[..., 1].double()) * OSF * f32(VS[1]) + f32(PCR[1])
        return torch.stack([x, y, c[..., 2].double()], dim=2)

    lo, hi = torch.tensor(lim[:3], dtype=torch.float64, device="cuda"), torch.tensor(lim[3:], dtype=torch.float64, device="cuda")
    valid = torch.arange(k, device="cuda")[None, :] < seg_len[:, None]
    ctr = centres(cand)
    near = (((ctr - lo).abs() <= 1e-5) | ((ctr - hi).abs() <= 1e-5)).any(dim=2)
    cand[near] = torch.tensor([0.5, 0.5, 0.0, 0, 0, 0, 0, 1, 0, 0], device="cuda")      # moved off the limit (no cell centre lies on one)
    ctr = centres(cand)
    near = (((ctr - lo).abs() <= 1e-5) | ((ctr - hi).abs() <= 1e-5)).any(dim=2) & valid
    print(f"  candidates within 1e-5 of a range limit: {int(near.sum())} of {int(valid.sum())}")
    assert int(near.sum()) <= 1e-3 * int(valid.sum()) and int(near.sum()) == 0
    ok = ((ctr >= lo) & (ctr <= hi)).all(dim=2) & valid
    want_len = ok.sum(dim=1)
    lost = want_len < seg_len
    share = 1.0 - float(ok.sum()) / float(valid.sum())
    print(f"  the range cuts {share:.3f} of the candidates; lists that lose one: {int(lost.sum())} of {S}")
    assert 0.2 < share < 0.7 and int(lost.sum()) > 0 and not bool(lost[central].any()) and int((~lost & (seg_len == k)).sum()) >= B_C2
    c64 = cand.double()
    box9 = torch.cat([ctr, torch.exp(c64[..., 3:6]), c64[..., 8:10], torch.atan2(c64[..., 6], c64[..., 7]).unsqueeze(2)], dim=2)
    tdesc = torch.frombuffer(bytearray(b"".join(_descs(lim))), dtype=torch.uint8).cuda()
    full_losing = next(s for s in range(S) if lens[s] == k and bool(lost[s]))
    tot_a = torch.where(central, torch.full_like(seg_len, 5000), seg_len)                 # only lists that lose nothing are cut at pre_max
    tot_b = tot_a.clone()
    tot_b[full_losing] = k + 1                                                            # one cut list loses a candidate
    tot_c = seg_len.clone()                                                               # no list is cut
    srt = torch.sort((~ok).to(torch.int8), dim=1, stable=True)[1]                          # survivors first, in order
    for name, tot, want_flag in (("cut lists lose nothing", tot_a, 0), ("one cut list loses", tot_b, 1), ("no list is cut", tot_c, 0)):
        assert want_flag == int(bool((lost & (tot > k)).any()))
        ln = seg_len.clone()
        boxes9 = torch.full((S * k, 9), -7.0, device="cuda")
        boxes7 = torch.full((S * k, 7), -7.0, device="cuda")
        scores = torch.full((S * k,), -7.0, device="cuda")
        flag = torch.zeros((1,), dtype=torch.int32, device="cuda")
        check(L.pnx_decode_boxes_lazy(ptr(tdesc), ptr(koff), len(NCLS), nct, ptr(skeys), ptr(order), ptr(seg_start), ptr(ln), ptr(tot.contiguous()), S, k,
                                      ptr(cand), ptr(boxes9), ptr(boxes7), ptr(scores), ptr(flag), stream_ptr()), "pnx_decode_boxes_lazy")
        assert int(flag) == want_flag, (name, int(flag))
        assert torch.equal(ln.long(), want_len), (name, (ln.long() != want_len).nonzero().flatten()[:8].tolist())
        keep = torch.arange(k, device="cuda")[None, :] < want_len[:, None]
        assert torch.equal(scores.view(S, k)[keep].view(torch.int32), torch.gather(sc, 1, srt)[keep].view(torch.int32)), (name, "survivors / order / scores")
        wb = torch.gather(box9, 1, srt[..., None].expand(S, k, 9))[keep]
        gb = boxes9.view(S, k, 9)[keep].double()
        err = ((gb - wb).abs() / (1e-4 + 1e-4 * wb.abs())).max().item()
        g7 = boxes7.view(S, k, 7)[keep]
        assert torch.equal(g7[:, :6], boxes9.view(S, k, 9)[keep][:, :6]) and torch.equal(g7[:, 6], boxes9.view(S, k, 9)[keep][:, 8])
        print(f"  {name}: flag {int(flag)}, {int(keep.sum())} survivors, worst box error / (1e-4 + 1e-4 |ref|) {err:.4f}")
        assert err <= 1.0 and int(keep.sum()) > 0


# ---------------------------------------------------------------------------------------------------- the decoder as one call (pnx_decode_lazy_enqueue)

def test_lazy_enqueue_equals_the_step_by_step_path_over_three_batches():
    """PackedDecoder.launch_lazy_fused (pnx_decode_lazy_enqueue: keys, top-k, cells, k_sephead_lazy, boxes, NMS, gather out of persistent scratch) against
    launch_lazy with ops.sephead_lazy as evaluator (fresh buffers per step) at the C2 shape: out, counts and flag bit-identical over three consecutive batches --
    sparse maps (short lists), dense maps (every list full; candidates near the border fail the range test: flag), dense maps whose border is masked out (full
    lists, nothing lost) -- so that every persistent scratch buffer is stale when the next batch arrives."""
    from pillarnext_amd import ops
    from pillarnext_amd.decode import PackedDecoder

    B, H, W, T = B_C2, H_C2, W_C2, len(NCLS)
    cfg = dict(nms=dict(nms_pre_max_size=PRE_MAX, nms_post_max_size=POST_MAX, nms_iou_threshold=[[0.2], [0.2, 0.2], [0.2, 0.25], [0.2], [0.2, 0.2], [0.2, 0.2]]),
               score_threshold=0.1, pc_range=list(PCR), voxel_size=list(VS), out_size_factor=[OSF] * T, post_center_limit_range=[-50.0, -50.0, -10.0, 50.0, 50.0, 10.0])
    rect = [[0.5] * nc for nc in NCLS]
    g = torch.Generator(device="cuda").manual_seed(51)
    tasks = []
    for ti in range(T):
        W1, b1, W2, b2 = _lazy_weights(200 + ti, torch.bfloat16)
        up = torch.randn((B, H, W, 64), device="cuda", generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
        tasks.append((up, ops.conv3x3_pack_weights(W1), b1, ops.sephead_lazy_pack_w2(_w2m(W2)), b2))

    def maps(mean, border):
        out = []
        for _ in range(T):
            x = torch.randn((B, H, W, 16), device="cuda", generator=g)
            x[..., 1:] = x[..., 1:] * 1.2 + mean
            if border:
                x[:, :40, :, 1:], x[:, -40:, :, 1:], x[:, :, :40, 1:], x[:, :, -40:, 1:] = -20.0, -20.0, -20.0, -20.0
            out.append(x.to(torch.bfloat16).permute(0, 3, 1, 2))
        return out

    batches = [maps(-6.5, False), maps(-2.19, False), maps(-2.19, True)]
    fused, plain = PackedDecoder(NCLS, rect, cfg, True, [16] * T), PackedDecoder(NCLS, rect, cfg, True, [16] * T)
    lens = {}

    def evaluator(local, seg_len, valid, segs):
        lens["len"] = seg_len.clone()
        return ops.sephead_lazy(tasks, CLASS_TASK, B, local.contiguous(), seg_len, PRE_MAX)

    def take(pend):
        pend.event.synchronize()
        r = (pend.out_h.clone(), pend.cnt_h.clone(), int(pend.flag_h[0]))
        pend.done = True
        return r

    flags = []
    for i, dense in enumerate(batches):
        a = take(fused.launch_lazy_fused(dense, tasks, CLASS_TASK))
        b = take(plain.launch_lazy(dense, evaluator))
        ln = lens["len"]
        print(f"lazy_enqueue batch {i}: candidates per list {int(ln.min())} .. {int(ln.max())} (sum {int(ln.sum())}), flag {b[2]}, detections {int(b[1].sum())}")
        assert a[2] == b[2], (i, "flag", a[2], b[2])
        assert torch.equal(a[1], b[1]), (i, "counts", (a[1] != b[1]).nonzero().flatten()[:8].tolist())
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (i, "out")
        assert int(b[1].sum()) > 0
        flags.append(b[2])
        if i == 0:
            assert 0 < int(ln.max()) < PRE_MAX
        else:
            assert int(ln.min()) == PRE_MAX
    assert flags == [0, 1, 0], flags
    assert any(key[0] == "lazy_fused" for key in fused._dev)

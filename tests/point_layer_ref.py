"""fp64 twin of the per-point training layer of the multi-view reader (csrc/point_layer_train.hip behind ops.PointLayer) -- test helper, plain numpy
on the CPU, no kernel code.

Forward, n rows, cin -> cout channels, an optional cell index inv (n) in [0, G):
    z = x W^T      mean, var = mean and BIASED variance of z over the rows      is = 1 / sqrt(var + eps)      xhat = (z - mean) is
    pre = xhat gamma + beta      y = relu(pre)      gmax[g] = max of y over the rows of cell g (0 for a cell without a row)
    argmax[g] = the lowest row of cell g that attains the maximum (n for a cell without a row): pnx_scatter_max's contract
    running statistics by BatchNorm1d's rule: (1 - m) old + m new, the variance times n / (n - 1).
Backward for the upstream gradients dy (n, cout) and / or dgmax (G, cout), which add:
    dz = (dy + dgmax routed to the arg-max row) where pre > 0      dbeta = D1 = sum dz      dgamma = D2 = sum dz xhat
    dxpre = gamma is (dz - D1 / n - xhat D2 / n)      dx = dxpre W      dW = dxpre^T x.

Bars.  Next to every quantity q the twin returns q_terms, the sum of |terms| of its plain statement with the products expanded as
tests/pfn_train_ref.py expands them (|z| stands for sum_k |x_k w_k|, |xhat| for (|z| + |mean|) is, a BatchNorm output for |xhat gamma| + |gamma| +
|beta|, a sum over rows for the sum of the rows' terms), and q_bar = BN_REL * q_terms with BN_REL = 2^-16, the project's masked-BN ceiling
(tests/pfn_train_ref.py, test_gpu_train_kernels_at_scale.py) -- taken from the project, not measured on the node.  The statistics are held to the
masked-BN module's own denominators: 2^-16 (|mean| + std) and 2^-16 * 2 var.

Fragile decisions, as the project handles them.  A ReLU gate (row, channel) is ambiguous where |pre| <= its forward bar.  A cell maximum
(cell, channel) is ambiguous where the largest pre-activation of the cell is open and lies within its bar of 0, or the two largest DISTINCT rows
(bit-equal rows of one cell count as one: whichever of them is named, every per-row quantity is the same number -- the first-row rule decides and is
asserted) lie within the sum of their bars; a cell whose maximum is a closed gate is not ambiguous -- its gradient is 0 whichever row is named --
unless one of its rows is within its own bar of opening.  The tests zero the upstream gradient on these sets and assert their share."""
import numpy as np

EPS = 1e-3
U = 2.0 ** -24
BN_REL = 2.0 ** -16


def forward(x, W, gamma, beta, inv=None, G=0, eps=EPS):
    """x (n, cin), W (cout, cin), gamma, beta (cout): fp32 values, taken to fp64.  Returns a dict of values, *_terms and *_bar."""
    x32 = np.ascontiguousarray(x, np.float32)
    x, W, ga, be = (np.asarray(a, np.float64) for a in (x32, W, gamma, beta))
    n, cout = x.shape[0], W.shape[0]
    z, Zt = x @ W.T, np.abs(x) @ np.abs(W).T
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    is_ = 1.0 / np.sqrt(var + eps)
    xh, XA = (z - mean) * is_, (Zt + np.abs(mean)) * is_
    pre = xh * ga + be
    y_terms = XA * np.abs(ga) + np.abs(ga) + np.abs(be)
    y_bar = BN_REL * y_terms
    y = np.maximum(pre, 0.0)
    s = dict(n=n, cin=x.shape[1], cout=cout, x=x, W=W, gamma=ga, beta=be, eps=eps, z=z, mean=mean, var=var, invstd=is_, xhat=xh, XA=XA, pre=pre, y=y,
             y_terms=y_terms, y_bar=y_bar, gate_amb=np.abs(pre) <= y_bar, inv=None, G=0)
    unb = n / max(n - 1.0, 1.0)
    sd = np.sqrt(var)
    s.update(mean_bar=BN_REL * (np.abs(mean) + sd), var_bar=BN_REL * 2 * var, running_mean=mean, running_var=var * unb,
             running_mean_bar=BN_REL * (np.abs(mean) + sd), running_var_bar=BN_REL * 2 * var * unb)
    if inv is None:
        return s
    inv = np.asarray(inv, np.int64)
    rows = np.arange(n)[:, None]
    cols = np.arange(cout)[None, :]
    top = np.full((G, cout), -np.inf)
    np.maximum.at(top, inv, pre)
    has = np.bincount(inv, minlength=G) > 0
    # the lowest row that attains the maximum of y (all rows of a closed cell hold y = 0: its lowest row)
    ymax = np.zeros((G, cout))
    np.maximum.at(ymax, inv, y)
    arg = np.full((G, cout), n, np.int64)
    np.minimum.at(arg, inv, np.where(y == ymax[inv], rows, n))
    gmax = np.where(has[:, None], ymax, 0.0)
    ebar = np.zeros((G, cout))
    np.maximum.at(ebar, inv, y_bar)                                    # ReLU and the maximum are 1-Lipschitz: the largest bar of the cell
    tterms = np.zeros((G, cout))
    np.maximum.at(tterms, inv, y_terms)
    # the largest pre-activation among the OTHER distinct rows of the cell
    key = np.concatenate([inv[:, None], np.ascontiguousarray(x32).view(np.uint32).astype(np.int64)], axis=1)
    _, first_idx = np.unique(key, axis=0, return_index=True)
    first = np.zeros(n, bool)
    first[first_idx] = True
    argp = np.full((G, cout), n, np.int64)                             # first row that attains the largest pre-activation
    np.minimum.at(argp, inv, np.where(pre == top[inv], rows, n))
    p2 = np.where(first[:, None], pre, -np.inf)
    ok = has[:, None] & np.ones((1, cout), bool)
    p2[argp[ok], np.broadcast_to(cols, (G, cout))[ok]] = -np.inf
    sec = np.full((G, cout), -np.inf)
    np.maximum.at(sec, inv, p2)
    e_top = np.where(has[:, None], y_bar[np.minimum(argp, n - 1), cols], 0.0)
    near_open = np.full((G, cout), -np.inf)
    np.maximum.at(near_open, inv, pre + y_bar)
    opened = top > 0
    with np.errstate(invalid="ignore"):                                # -inf - -inf on the cells without a row
        max_amb = has[:, None] & np.where(opened, (top <= e_top) | (top - sec <= e_top + ebar), near_open >= 0)
    s.update(inv=inv, G=G, has=has, top=top, gmax=gmax, gmax_terms=tterms, gmax_bar=ebar, argmax=arg, max_amb=max_amb, max_open=has[:, None] & opened)
    return s


def backward(s, dy=None, dgmax=None):
    """dgamma, dbeta, dW, dx (+ _terms, _bar) for upstream gradients the caller has zeroed on s['gate_amb'] (dy) and s['max_amb'] (dgmax)."""
    n, cout = s["n"], s["cout"]
    dz = np.zeros((n, cout))
    dzt = np.zeros((n, cout))
    if dy is not None:
        dy = np.asarray(dy, np.float64)
        dz += dy
        dzt += np.abs(dy)
    if dgmax is not None:
        dg = np.asarray(dgmax, np.float64)
        live = s["has"][:, None] & np.ones((1, cout), bool)
        r, c = s["argmax"][live], np.broadcast_to(np.arange(cout)[None, :], dg.shape)[live]
        dz[r, c] += dg[live]
        dzt[r, c] += np.abs(dg[live])
    gate = s["pre"] > 0
    dz, dzt = dz * gate, dzt * gate
    xh, XA, x, W = s["xhat"], s["XA"], s["x"], s["W"]
    D1, D1t = dz.sum(0), dzt.sum(0)
    D2, D2t = (dz * xh).sum(0), (dzt * XA).sum(0)
    a = s["gamma"] * s["invstd"]
    dxp = a * (dz - D1 / n - xh * D2 / n)
    dxpt = np.abs(a) * (dzt + D1t / n + XA * D2t / n)
    out = dict(dbeta=D1, dbeta_terms=D1t, dgamma=D2, dgamma_terms=D2t, dW=dxp.T @ x, dW_terms=dxpt.T @ np.abs(x), dx=dxp @ W, dx_terms=dxpt @ np.abs(W),
               dz=dz)
    for k in ("dbeta", "dgamma", "dW", "dx"):
        out[k + "_bar"] = BN_REL * out[k + "_terms"]
    return out


def make_case(n, cin, cout, seed, offset=0.0, G=None, cells="random", dup=0):
    """Seeded fp32 inputs: x ~ N(offset, 1), W ~ N(0, 1 / cin), gamma ~ U(0.5, 1.5), beta ~ N(0, 0.25).  cells: "random" (G cells, some empty when
    G is large), "one" (one cell holds every row), "each" (one row per cell); dup: that many rows copied bit for bit onto later rows of cell 0."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, cin)) + offset).astype(np.float32)
    W = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    beta = (0.5 * rng.standard_normal(cout)).astype(np.float32)
    inv = None
    if cells == "one":
        G, inv = 1, np.zeros(n, np.int64)
    elif cells == "each":
        G, inv = n, rng.permutation(n).astype(np.int64)
    elif G is not None:
        inv = rng.integers(0, G, n).astype(np.int64)
    if dup:
        src = rng.choice(n // 2, dup, replace=False)
        dst = n // 2 + rng.choice(n - n // 2, dup, replace=False)
        x[dst] = x[src]
        inv[src] = 0
        inv[dst] = 0
    return dict(x=x, W=W, gamma=gamma, beta=beta, inv=inv, G=G or 0)

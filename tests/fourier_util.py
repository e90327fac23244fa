"""The fp64 reference of the sine-first-layer network (pinn_hip.h: PINN_ACT_SIN_TANH) and the cases the Fourier tests share.

The network: a_1 = sin(W_0 x + b_0), tanh on every other hidden layer, the last layer bare — written here in torch from the
flat parameter vector, independent of the kernels.  Jets by oracle.pinn_oracle.compute_gradient, the residuals by the
oracle's own field formulas, the fidelity MSE as oracle.fidelity_loss forms it, gradients by autograd.  Parameters and
inputs are rounded to fp32 FIRST, so the fp64 evaluation, the fp32 CPU evaluation (the yardstick) and the kernels see the
same numbers.

Error measure: err(q, q64) = max|q - q64| / max|q64|.  Bar of a quantity: the larger of the bar tests/test_engine_gpu.py
uses for it on the tanh network (Y / dY 2e-6, term sums 2e-6, gradient 2e-5) and 4 x the error of the yardstick — the same
formula evaluated by torch in fp32 on the CPU against its fp64 self — on the same case.
"""
import functools
import math

import torch

from oracle import pinn_oracle as O

SIBLING_BAR = {"Y": 2e-6, "dY": 2e-6, "sums": 2e-6, "grad": 2e-5}

RES = {
    # residual: (input names, output names, k)
    "Navier_Stokes": (("t", "x", "y"), ("h", "z", "u", "v"), 3),
    "physics_equation": (("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"), 2),
    "continuity_only": (("x", "y"), ("U", "V", "h"), 2),
    "continuity_ftemp": (("x", "y"), ("U", "V", "h"), 2),
}
THRESHOLD, ANCHOR = 25.5, 0.75


def err(q, q64) -> float:
    q64 = torch.as_tensor(q64).double().cpu()
    return float((torch.as_tensor(q).double().cpu() - q64).abs().max() / q64.abs().max().clamp_min(1e-300))


def bar(kind: str, yard: float) -> float:
    return max(SIBLING_BAR[kind], 4.0 * yard)


def sin_mlp(params, x):
    """Linear -> sin on hidden layer 0, Linear -> tanh on the others, last Linear bare."""
    n_lin = len(params) // 2
    a = x
    for i in range(n_lin):
        a = torch.nn.functional.linear(a, params[2 * i], params[2 * i + 1])
        if i < n_lin - 1:
            a = torch.sin(a) if i == 0 else torch.tanh(a)
    return a


def make_params(layers, sigma, seed, out_scale=1.0):
    """fp32 parameters: W_0 ~ N(0, sigma^2), b_0 ~ U[0, 2 pi) (a random phase), Xavier-uniform weights and NON-ZERO biases
    U(-0.3, 0.3) on every other hidden layer, the last layer Xavier / nn.Linear default, its weights times out_scale."""
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(layers, "xavier", g)
    params[0] = torch.empty_like(params[0]).normal_(0.0, float(sigma), generator=g)
    params[1] = torch.empty_like(params[1]).uniform_(0.0, 2.0 * math.pi, generator=g)
    for i in range(1, len(layers) - 2):
        params[2 * i + 1] = torch.empty_like(params[2 * i + 1]).uniform_(-0.3, 0.3, generator=g)
    params[-2] = params[-2] * out_scale
    return params


def points(N, d_in, seed):
    return torch.rand(N, d_in, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def jet(params, X, grad_cols, dtype=torch.float64):
    """Y (N, d_out), dY (k, N, d_out) in `dtype`."""
    p = [q.to(dtype) for q in params]
    cols = O.split_columns(X.to(dtype), grad_cols)
    Y = sin_mlp(p, torch.cat(cols, dim=-1))
    if not grad_cols:
        return Y.detach(), torch.zeros(0, *Y.shape, dtype=dtype)
    dY = torch.stack([torch.cat([O.compute_gradient(Y[:, c:c + 1], cols[j]) for c in range(Y.shape[1])], dim=1)
                      for j in grad_cols])
    return Y.detach(), dY.detach()


def fields(residual, cols, Y):
    """The residual's fields from the oracle's formulas (inputs and outputs in the residual's own argument order)."""
    outs = [Y[:, o:o + 1] for o in range(len(RES[residual][1]))]
    if residual == "Navier_Stokes":
        return O.navier_stokes_fields(*cols[:3], *outs)
    if residual == "physics_equation":
        return O.physics_equation_fields(*cols[:2], *outs)
    U, V, h = outs
    return (O.continuity_fields(cols[0], cols[1], h, U, V),)


def term_sums(residual, params, X, grad_cols, n_res=None):
    """The engine's term sums (sum over points of each squared field) as differentiable fp tensors of params' dtype.
    continuity_only: [sum fc^2, sum_{x < 25.5} (h - 0.75)^2, count]."""
    X = X if n_res is None else X[:n_res]
    cols = O.split_columns(X, grad_cols)
    Y = sin_mlp(params, torch.cat(cols, dim=-1))
    fs = fields(residual, cols, Y)
    sums = [(f ** 2).sum() for f in fs]
    if residual == "continuity_only":
        m = (X[:, 0:1] < THRESHOLD).to(X.dtype)
        sums += [(m * (Y[:, 2:3] - ANCHOR) ** 2).sum(), m.sum()]
    return torch.stack(sums)


def point_fields(residual, params, X, grad_cols):
    """(rows, N): the residual's fields at every point (continuity_only: and h - 0.75 where x < 25.5, else 1)."""
    cols = O.split_columns(X, grad_cols)
    Y = sin_mlp(params, torch.cat(cols, dim=-1))
    fs = list(fields(residual, cols, Y))
    if residual == "continuity_only":
        m = X[:, 0:1] < THRESHOLD
        fs.append(torch.where(m, Y[:, 2:3] - ANCHOR, torch.ones_like(Y[:, 2:3])))
    return torch.cat(fs, dim=1).t().detach()


def point_condition(residual, params, X, grad_cols, seed):
    """Per point: the largest relative change of a field, in units of 2^-23, when every parameter moves by a relative
    +-2^-23 (random signs) — how many roundings of a field one rounding of the parameters makes.  fp64 only."""
    g = torch.Generator().manual_seed(seed)
    p0 = [q.double() for q in params]
    p1 = [q * (1.0 + (torch.randint(0, 2, q.shape, generator=g).double() * 2 - 1) * 2.0 ** -23) for q in p0]
    a, b = point_fields(residual, p0, X.double(), grad_cols), point_fields(residual, p1, X.double(), grad_cols)
    return ((b - a).abs() / a.abs().clamp_min(1e-300)).max(dim=0).values / 2.0 ** -23


def mse_sums(params, X, T, out_cols, n0=0):
    """Per target column: sum over the points from n0 on of (true - pred)^2 (oracle.fidelity_loss without its means)."""
    Y = sin_mlp(params, X[n0:])
    return torch.stack([((T[:, j:j + 1] - Y[:, o:o + 1]) ** 2).sum() for j, o in enumerate(out_cols)])


def scales(residual, X, N_res):
    """term_scale of a residual request on the first N_res rows of X: 1 / N per term (continuity_only: its own counts)."""
    if residual == "continuity_only":
        cnt = max(float((X[:N_res, 0] < THRESHOLD).sum()), 1.0)
        return torch.tensor([1.0 / N_res, 1.0 / cnt, 0.0])
    return torch.full((len(fields_count(residual)),), 1.0 / N_res)


def fields_count(residual):
    return {"Navier_Stokes": (0, 1, 2), "physics_equation": (0, 1, 2), "continuity_only": (0, 1, 2), "continuity_ftemp": (0,)}[residual]


def loss_and_grad(params, X, dtype, residual=None, grad_cols=(), scale=None, T=None, out_cols=(), col_scale=None, n_split=-1):
    """(term sums or None, column sums or None, flat gradient of  scale . term_sums + col_scale . col_sums) in `dtype`.
    n_split < 0: every term on every point; >= 0: the residual on the first n_split points, the fidelity columns on the rest."""
    p = [q.to(dtype).requires_grad_(True) for q in params]
    Xd = X.to(dtype)
    total, ts, cs = 0, None, None
    if residual is not None and n_split == 0:       # a split request without collocation points: zero sums, no gradient
        ts = torch.zeros(len(scale), dtype=dtype)
    elif residual is not None:
        ts = term_sums(residual, p, Xd, grad_cols, None if n_split < 0 else n_split)
        total = total + (ts * scale.to(dtype)).sum()
    if T is not None:
        cs = mse_sums(p, Xd, T.to(dtype), out_cols, 0 if n_split < 0 else n_split)
        total = total + (cs * col_scale.to(dtype)).sum()
    g = O.flat_grad(total, p)
    return (None if ts is None else ts.detach()), (None if cs is None else cs.detach()), g.detach()


def blocks(layers):
    """Slices of the flat vector, block by block: W_0, b_0, a middle layer's W (if any) and the last layer's W."""
    offs, off = [], 0
    for i in range(len(layers) - 1):
        nw = layers[i] * layers[i + 1]
        offs.append((off, off + nw, off + nw + layers[i + 1])); off += nw + layers[i + 1]
    out = {"W0": slice(offs[0][0], offs[0][1]), "b0": slice(offs[0][1], offs[0][2])}
    if len(offs) > 2:
        mid = offs[len(offs) // 2 if len(offs) > 3 else 1]
        out["Wmid"] = slice(mid[0], mid[1]); out["bmid"] = slice(mid[1], mid[2])
    out["Wlast"] = slice(offs[-1][0], offs[-1][1]); out["blast"] = slice(offs[-1][1], offs[-1][2])
    return out


@functools.lru_cache(maxsize=None)
def loss_case(kind, L, W, N, sigma=1.0):
    """One case of the loss tests, with its fp64 reference and its fp32 yardstick (computed once, shared by the engines).
    kind: ns | pe | co (residual_loss_grad), mse, merged (residual + fidelity on every point), split.
    sigma: the constructor's default fourier_sigma (the jet tests carry sigma = 1 and 16; with the random phase |z_0| reaches 8
    either way, and one fp32 rounding of such a z is 5e-7 of sin z whatever evaluates it)."""
    residual = {"ns": "Navier_Stokes", "pe": "physics_equation", "co": "continuity_only", "mse": None,
                "merged": "physics_equation", "split": "physics_equation"}[kind]
    res_for_shape = residual or "physics_equation"
    inn, outn, k = RES[res_for_shape]
    d_in, d_out = len(inn), len(outn)
    layers = [d_in] + [W] * L + [d_out]
    grad_cols = tuple(range(k)) if kind != "mse" else ()

    def draw_points(M):
        Xc = points(M, d_in, seed0 + 7)
        if residual == "continuity_only":
            Xc[:, 0] = Xc[:, 0] * 40
        return None, Xc

    def draw(seed):
        # physics_equation divides by rho (eta_mean + h): keep the outputs near the last layer's biases, h = 0.75 and eta_mean = 0
        params = make_params(layers, sigma, seed, out_scale=0.2 if res_for_shape == "physics_equation" else 1.0)
        if res_for_shape == "physics_equation":
            params[-1][outn.index("h")] = 0.75
            params[-1][outn.index("eta_mean")] = 0.0
        X = points(N, d_in, seed + 1)
        if residual == "continuity_only":
            X[:, 0] = X[:, 0] * 40          # make x < 25.5 a real subset
        return params, X

    # A term sum over a few points can be a small difference of large derivatives (one point: fc = u_x + v_y alone; measured
    # on plain draws at N = 1: 8 to 2700 roundings of the sum per rounding of the parameters), and its RELATIVE error then
    # measures that cancellation, not a kernel — and the one-sample yardstick of such a case is as likely small as large.  So
    # the N points of a residual case are the N best conditioned of max(4 N, 1024) candidates drawn the same way — a property
    # of the fp64 reference alone, decided before any kernel runs (point_condition).  The bars are the ones they were.
    seed0 = 1000 * L + 10 * W + N
    n_res_pts = N if kind != "split" else (N - max(1, N // 4) if N > 1 else 0)
    params, X = draw(seed0)
    cond = 0.0
    if residual is not None and n_res_pts > 0:
        _, Xc = draw_points(max(4 * N, 1024))
        c = point_condition(residual, params, Xc, grad_cols, seed0)
        keep = torch.sort(torch.argsort(c)[:N]).values
        X, cond = Xc[keep].contiguous(), float(c[keep].max())
    n_split = -1
    T = out_cols = col_scale = scale = None
    n_res = N
    seed = seed0
    if kind in ("mse", "merged", "split"):
        out_cols = [0, 1, 4]
        if kind == "split":
            n_split = n_res_pts
            n_res = n_split
        n_fid = N if n_split < 0 else N - n_split
        # targets at a distance of 0.5 to 1 from the prediction, either side: (true - pred)^2 is then no small difference (with
        # true ~ U(0, 1) a single point's column sum can be: the same conditioning argument as above, from fp64 alone)
        gT = torch.Generator().manual_seed(seed + 2)
        Yf = jet(params, X[N - n_fid:], (), torch.float64)[0][:, out_cols]
        T = (Yf + (torch.rand(n_fid, 3, generator=gT).double() * 0.5 + 0.5) * (torch.randint(0, 2, (n_fid, 3), generator=gT).double() * 2 - 1)).float()
        col_scale = torch.tensor([1.0, 2.0, 0.5]) / n_fid
    if residual is not None:
        scale = scales(residual, X, n_res) if n_res > 0 else torch.zeros(3)
    ref = loss_and_grad(params, X, torch.float64, residual, grad_cols, scale, T, out_cols, col_scale, n_split)
    y32 = loss_and_grad(params, X, torch.float32, residual, grad_cols, scale, T, out_cols, col_scale, n_split)
    return dict(kind=kind, residual=residual, inn=inn, outn=outn, layers=layers, params=params, X=X, grad_cols=grad_cols,
                scale=scale, T=T, out_cols=out_cols, col_scale=col_scale, n_split=n_split, ref=ref, y32=y32, cond=cond)

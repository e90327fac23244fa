"""Non-finite propagation (tests/test_nonfinite_cpu.py, tests/test_nonfinite_gpu.py): the networks, the poison sites and
the reference — oracle/pinn_oracle.py in fp32 on the same poisoned data.

A NaN at one collocation point must make the loss sums and the gradient NaN (that is how a diverged run becomes visible), and
must stay inside its own row of the per-point outputs (a kernel that reads a neighbour's lane, lets a clamped tail lane into a
stored row, or selects a NaN away fails one of the two)."""
from __future__ import annotations

import functools
import math

import torch

from oracle import pinn_oracle as O
from tests.trained_state_util import trained_like

NS_OUT = ("h", "z", "u", "v")
PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
# the smallest shapes with a full 16-point tile, a second tile and a ragged tail; split requests: N_RES residual rows + N_FID
N_RES, N_FID = 37, 21
NETS = {
    # name: d_in, d_out, hidden layers, width, differentiated columns, residual, input names, output names, engines
    "pe_3x10": (2, 6, 3, 10, (0, 1), "physics_equation", ("x", "y"), PE_OUT, ("generic", "tile", "batch")),                       # padded width 16
    "ns_3x20_5in": (5, 4, 3, 20, (0, 1, 2), "Navier_Stokes", ("t", "x", "y", "u0", "v0"), NS_OUT, ("generic", "tile", "batch")),  # 32, two extra inputs
    "ns_3x48": (3, 4, 3, 48, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), NS_OUT, ("generic", "tile", "coop")),                   # 64
    "ns_2x128": (3, 4, 2, 128, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), NS_OUT, ("wide", "wide_bf16")),                       # the wide engine
}
FID_COLS = (1, 3)                     # the output columns of the fidelity rows' targets
TERM_SCALE = (1.0 / N_RES, 0.7 / N_RES, 1.3 / N_RES)
COL_SCALE = (0.5 / N_FID, 1.5 / N_FID)

# poison sites, one non-finite value each: (what, row, column); columns of X by role below
X_SITES = ("x0", "x16", "xlast", "xextra")          # rows 0, 16 and N_RES - 1 of a differentiated column; a plain input column
PARAM_SITES = ("w", "b")                            # one hidden weight, one hidden bias
SPLIT_ONLY = ("xfid_last", "t")                     # the last row of all (a fidelity row: what tail lanes are clamped to); one target
SITES = X_SITES + PARAM_SITES + SPLIT_ONLY


class Net:
    def __init__(self, name):
        self.name = name
        self.d_in, self.d_out, self.L, self.W, self.gc, self.res, self.inn, self.outn, self.engines = NETS[name]
        self.layers = O.layer_sizes(self.d_in, self.L, self.W, self.d_out)
        g = torch.Generator().manual_seed(4242 + len(name))
        self.params = trained_like(self.layers, g, residual=self.res, outn=self.outn)
        self.X = torch.rand(N_RES + N_FID, self.d_in, generator=g) * 2 - 1
        self.T = torch.randn(N_FID, len(FID_COLS), generator=g)
        from pinn_depthestimation_amd.engine import RESIDUAL_ROLES
        _, out_roles, dir_roles = RESIDUAL_ROLES[self.res]
        self.in_roles = [self.inn.index(r) for r in dir_roles]
        self.out_roles = [self.outn.index(r) for r in out_roles]

    def sites(self, split: bool):
        out = [s for s in X_SITES + PARAM_SITES if s != "xextra" or self.d_in > len(self.gc)]
        return out + list(SPLIT_ONLY) if split else out

    def desc(self, engine: str, **kw):
        from pinn_depthestimation_amd import NetDesc, _lib as L
        e = {"generic": L.ENGINE_GENERIC, "tile": L.ENGINE_FUSED_TILE, "batch": L.ENGINE_FUSED_BATCH, "coop": L.ENGINE_FUSED_COOP,
             "wide": L.ENGINE_WIDE, "wide_bf16": L.ENGINE_WIDE, "auto": L.ENGINE_AUTO}[engine]
        return NetDesc(self.d_in, self.d_out, self.L, self.W, self.gc, engine=e,
                       precision=L.PREC_BF16 if engine == "wide_bf16" else L.PREC_F32, **kw)

    def spec(self, **kw):
        from pinn_depthestimation_amd import ResidualSpec
        return ResidualSpec.from_names(self.res, self.inn, self.gc, self.outn, **kw)


@functools.lru_cache(maxsize=None)
def net(name) -> Net:
    return Net(name)


def poisoned(n: Net, site, value=math.nan):
    """(params, X, T) copies with `value` at the site (site None: clean copies)."""
    params, X, T = [p.clone() for p in n.params], n.X.clone(), n.T.clone()
    if site == "x0": X[0, n.gc[0]] = value
    elif site == "x16": X[16, n.gc[-1]] = value
    elif site == "xlast": X[N_RES - 1, n.gc[0]] = value
    elif site == "xextra": X[5, n.d_in - 1] = value
    elif site == "xfid_last": X[N_RES + N_FID - 1, n.gc[0]] = value
    elif site == "w": params[2][1, 2] = value
    elif site == "b": params[3][n.W - 1] = value
    elif site == "t": T[4, 1] = value
    else: assert site is None, site
    return params, X, T


def row_of(site):
    """The point a site in X poisons (per-point outputs), None for a parameter (every row)."""
    return {"x0": 0, "x16": 16, "xlast": N_RES - 1, "xextra": 5}.get(site)


# ---- forward and fields of the oracle, with variants (the extra tile-kernel requests) -----------------------------------------
def _mlp(q, x, sine):
    if not sine:
        return O.mlp_forward(q, x)
    from tests.fourier_util import sin_mlp
    return sin_mlp(q, x)


def fields_of(n: Net, q, X, variant="plain", coef=None):
    """The residual's signed fields, each (N, 1), of the oracle's formulas on the network q at the rows of X.
    variant: plain | corrected (physics_equation's corrected radiation stress) | coef (closure coefficient `coef`) | sine."""
    cols = O.split_columns(X, n.gc)
    Y = _mlp(q, torch.cat(cols, dim=-1), variant == "sine")
    ins, outs = [cols[i] for i in n.in_roles], [Y[:, o:o + 1] for o in n.out_roles]
    if variant == "corrected":
        from tests.pe_corrected_util import pec_fields
        return pec_fields(*ins, *outs)
    if variant == "coef":
        from tests.coef_util import formula
        return formula(n.res, coef, ins, outs)
    return (O.navier_stokes_fields if n.res == "Navier_Stokes" else O.physics_equation_fields)(*ins, *outs)


def oracle_loss(n: Net, params, X, T=None, split=False, variant="plain", weights=None, coef=None, dtype=torch.float32):
    """(term sums, column sums or None, flat gradient) in `dtype`: the residual on the first N_RES rows of X (all rows when
    not split), the fidelity columns on the rows behind; gradient of TERM_SCALE . term sums + COL_SCALE . column sums.
    weights: (N,) point weights on every squared field."""
    q = [p.detach().to(dtype).clone().requires_grad_(True) for p in params]
    X = X.to(dtype)
    Xr = X[:N_RES] if split else X
    f = fields_of(n, q, Xr, variant, coef)
    w = 1.0 if weights is None else weights.to(dtype).reshape(-1, 1)
    ts = torch.stack([(w * fi ** 2).sum() for fi in f])
    total = (ts * torch.tensor(TERM_SCALE, dtype=dtype)).sum()
    cs = None
    if split:
        Yf = _mlp(q, X[N_RES:], variant == "sine")
        cs = torch.stack([((T[:, j].to(dtype) - Yf[:, o]) ** 2).sum() for j, o in enumerate(FID_COLS)])
        total = total + (cs * torch.tensor(COL_SCALE, dtype=dtype)).sum()
    return ts.detach(), (None if cs is None else cs.detach()), O.flat_grad(total, q).detach()


def oracle_points(n: Net, params, X, dtype=torch.float32, variant="plain"):
    """(Y (N, d_out), dY (k, N, d_out), fields (3, N)) of the oracle in `dtype` at the rows of X."""
    q = [p.detach().to(dtype) for p in params]
    X = X.to(dtype)
    if variant == "sine":
        from tests.fourier_util import jet
        Y, dY = jet(q, X, n.gc, dtype)
    else:
        Y, dY = O.jet(q, X, n.gc)
    f = fields_of(n, q, X, variant)
    return Y, dY, torch.cat([t.detach() for t in f], dim=1).T.contiguous()


@functools.lru_cache(maxsize=None)
def reference_loss(name, site, split, variant="plain"):
    """The oracle in fp32 on the data poisoned at `site` (None: clean), computed once and shared; callers leave it unchanged."""
    n = net(name)
    params, X, T = poisoned(n, site)
    kw = {}
    if variant == "weighted":
        kw = dict(weights=point_weights())
    if variant == "coef":
        kw = dict(coef=torch.tensor(COEF[n.res]))
    return oracle_loss(n, params, X if split else X[:N_RES], T, split, "plain" if variant == "weighted" else variant, **kw)


@functools.lru_cache(maxsize=None)
def reference_points(name, site, value=math.nan, dtype=torch.float32, variant="plain"):
    n = net(name)
    params, X, _ = poisoned(n, site, value)
    return oracle_points(n, params, X[:N_RES], dtype, variant)


COEF = {"Navier_Stokes": 0.4, "physics_equation": 0.5}      # tests/coef_util.COEFS' second values


def point_weights():
    return torch.rand(N_RES, generator=torch.Generator().manual_seed(77)) + 0.5


# ---- comparing NaN patterns -----------------------------------------------------------------------------------------------------
def nan_mismatch(got: torch.Tensor, ref: torch.Tensor):
    """Indices where `got` is NaN and `ref` is not, or the other way round."""
    return torch.nonzero(torch.isnan(got.cpu().reshape(-1)) != torch.isnan(ref.reshape(-1))).reshape(-1).tolist()


def bits_differ(a: torch.Tensor, b: torch.Tensor):
    """Indices where two fp32 tensors differ bit for bit (two NaNs count as equal)."""
    a, b = a.cpu().reshape(-1), b.cpu().reshape(-1)
    same = (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
    return torch.nonzero(~same).reshape(-1).tolist()

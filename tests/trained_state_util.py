"""Shared by test_trained_state_cpu.py / test_trained_state_gpu.py: network states with NON-ZERO hidden biases, and a
gradient comparison that holds every parameter block (W_l, b_l) to the bound on its own.

Every other parity test starts from init_params / init_flat_params, which leave the bias of every hidden layer at exactly
zero (dnn.py:27-52): a kernel that dropped a hidden bias, read the neighbouring unit's, another layer's or another
ensemble member's would pass all of them.  And a whole-vector rel-L2 hides the bias blocks, which carry about 1e-2 of the
gradient's norm: a bias block that is 0.2 % wrong passes at 2e-5.

Two named states (STATES):
  biased      Xavier weights, hidden biases U(-0.5, 0.5).  Any shape.
  saturating  hidden weights x 3, hidden biases U(-1, 1): 11-40 % of the last hidden layer's activations exceed 0.99, which
              exercises tanh's |x| >= 0.625 branch and s = 1 - a^2 near saturation.  Only for at most 3 hidden layers: deeper
              nets are chaotic under it (40x20: the oracle's own fp32 run is 1.5e-1 off its fp64 run).
"""
import torch

from oracle import pinn_oracle as O

STATES = {"biased": dict(gain=1.0, bias=0.5), "saturating": dict(gain=3.0, bias=1.0)}
SATURATING_MAX_HIDDEN = 3
GAP_CAP = 5e-6      # the reference's own fp32-vs-fp64 difference per block must stay within this for every committed case


def trained_like(layers, generator, gain=1.0, bias=0.5, residual=None, outn=None, init_type="xavier"):
    """[W0, b0, W1, b1, ...] (float32): O.init_params, hidden weights x gain, every hidden bias U(-bias, bias) from the
    same generator (drawn after the init, layer by layer).  residual == "physics_equation" (with the network's output
    names) gets the sweep's conditioning: output weights x 0.25, bias of h 0.75, of eta_mean 0, of k 0.5 (eta_mean + h stays
    away from 0, where 1 / (rho (eta_mean + h)) is singular)."""
    params = O.init_params(layers, init_type, generator)
    n_lin = len(layers) - 1
    for i in range(n_lin - 1):
        params[2 * i] = params[2 * i] * gain
        params[2 * i + 1] = (torch.rand(layers[i + 1], generator=generator) * 2 - 1) * bias
    if residual == "physics_equation":
        outn = list(outn)
        params[-2] = params[-2] * 0.25
        b = params[-1].clone()
        b[outn.index("h")], b[outn.index("eta_mean")], b[outn.index("k")] = 0.75, 0.0, 0.5
        params[-1] = b
    return params


def param_blocks(layers):
    """[(name, start, stop)] of W0, b0, W1, ... in the flat parameter vector (O.flatten's order)."""
    out, off = [], 0
    for i in range(len(layers) - 1):
        nw = layers[i] * layers[i + 1]
        out.append((f"W{i}", off, off + nw)); off += nw
        out.append((f"b{i}", off, off + layers[i + 1])); off += layers[i + 1]
    return out


def block_errors(got, ref, layers):
    """{block name: rel-L2 of got against ref within the block} (inf where ref's block is zero and got's is not)."""
    got, ref = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    out = {}
    for name, a, b in param_blocks(layers):
        rn = float(ref[a:b].norm())
        dn = float((got[a:b] - ref[a:b]).norm())
        out[name] = dn / rn if rn > 0 else (0.0 if dn == 0 else float("inf"))
    return out


def assert_blocks_close(got, g64, g32, layers, what, floor=2e-5, gap_mult=4.0, gap_cap=GAP_CAP):
    """Every block of `got` within max(floor, gap_mult * gap) of g64 in rel-L2, gap = the block's rel-L2 of g32 (the
    reference's own fp32 run) against g64: tests/test_engine_gpu.py's rule, per block.  A block whose fp64 norm is 0 must
    be at most 1e-12 |g64| in got.  The reference alone must be within gap_cap in every block (a condition on the CASE, not
    a tolerance; gap_cap=None where g32 is no fp32 run of the reference).  Returns {block: error}."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    g64 = torch.as_tensor(g64).detach().double().cpu().reshape(-1)
    g32 = torch.as_tensor(g32).detach().double().cpu().reshape(-1)
    n = sum(layers[i] * layers[i + 1] + layers[i + 1] for i in range(len(layers) - 1))
    assert got.numel() == g64.numel() == g32.numel() == n, (what, got.numel(), g64.numel(), g32.numel(), n)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries"
    total = float(g64.norm())
    errs, gaps, bad = {}, {}, []
    for name, a, b in param_blocks(layers):
        rn = float(g64[a:b].norm())
        if rn == 0.0:
            gaps[name] = 0.0
            errs[name] = float(got[a:b].norm())
            if errs[name] > 1e-12 * total:
                bad.append(f"{name} (fp64 block is zero, got norm {errs[name]:.2e})")
            continue
        gaps[name] = float((g32[a:b] - g64[a:b]).norm()) / rn
        errs[name] = float((got[a:b] - g64[a:b]).norm()) / rn
        if gap_cap is not None:
            assert gaps[name] <= gap_cap, (f"{what}: the reference's own fp32-fp64 gap in {name} is {gaps[name]:.2e} > {gap_cap:.0e}: "
                                           "a badly chosen case")
        if not errs[name] < max(floor, gap_mult * gaps[name]):
            bad.append(f"{name} ({errs[name]:.2e} > {max(floor, gap_mult * gaps[name]):.2e})")
    if bad:
        table = ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
        raise AssertionError(f"{what}: block(s) out of bound: {'; '.join(bad)}.  Every block: {table}")
    return errs


def worst(errs):
    """(block name, error) of the largest entry."""
    k = max(errs, key=errs.get)
    return k, errs[k]


# ---- the cases both modules use ------------------------------------------------------------------------------------------
NS_IO = (("t", "x", "y"), ("h", "z", "u", "v"))
PE_IO = (("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"))
CF_IO = (("x", "y"), ("U", "V", "h"))
CASES = {
    # name: (d_in, d_out, hidden, width, grad_cols, residual, in names, out names)
    "ns_8x64": (3, 4, 8, 64, (0, 1, 2), "Navier_Stokes") + NS_IO,          # width-64 epilogues, k-step-major I/O
    "pe_8x64": (2, 6, 8, 64, (0, 1), "physics_equation") + PE_IO,
    "pe_10x10": (2, 6, 10, 10, (0, 1), "physics_equation") + PE_IO,        # padded width 16, k = 2 (K1 = 3)
    "ns_3x12": (3, 4, 3, 12, (0, 1, 2), "Navier_Stokes") + NS_IO,          # padded width 16, k = 3 (K1 = 4)
    "cf_3x32": (2, 3, 3, 32, (0, 1), "continuity_ftemp") + CF_IO,          # padded width 32, K1 = 3
    "ns_5in": (5, 4, 3, 20, (0, 1, 2), "Navier_Stokes", ("t", "x", "y", "u0", "v0"), ("h", "z", "u", "v")),   # width 32, K1 = 4
    "cf_40x20": (2, 3, 40, 20, (0, 1), "continuity_ftemp") + CF_IO,        # gradient copies in the workspace, not LDS
    "co_3x64": (2, 3, 3, 64, (0, 1), "continuity_only") + CF_IO,
    "ns_out_first_3x12": (3, 7, 3, 12, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"),
                          ("aux0", "aux1", "h", "z", "u", "v", "aux2")),   # generic epilogue, output column 0 is no role
    "co_40x20": (2, 3, 40, 20, (0, 1), "continuity_only") + CF_IO,         # the ensemble's deep case
    "pe_4x48": (2, 6, 4, 48, (0, 1), "physics_equation") + PE_IO,          # the dropout instance's shape
    # the wide engine (64 < width <= 256)
    "ns_3x128": (3, 4, 3, 128, (0, 1, 2), "Navier_Stokes") + NS_IO,
    "cf_2x256": (2, 3, 2, 256, (0, 1), "continuity_ftemp") + CF_IO,
    "co_2x100": (2, 3, 2, 100, (0, 1), "continuity_only") + CF_IO,
    "ns_5x256": (3, 4, 5, 256, (0, 1, 2), "Navier_Stokes") + NS_IO,
}
N_POINTS = 777      # ragged for every tile size (16, 64, 128)


class Case:
    """One network at one named state with its points: layers, params (list, float32), X (N, d_in) on the CPU, the
    residual's name and the network's input / output names."""

    def __init__(self, name, state, N=N_POINTS, seed=1234):
        self.d_in, self.d_out, self.L, self.W, self.gc, self.res, self.inn, self.outn = CASES[name]
        if state == "saturating":
            assert self.L <= SATURATING_MAX_HIDDEN, f"{name}: the saturating state is for at most {SATURATING_MAX_HIDDEN} hidden layers"
        g = torch.Generator().manual_seed(seed)
        self.name, self.state, self.N = name, state, N
        self.layers = O.layer_sizes(self.d_in, self.L, self.W, self.d_out)
        self.params = trained_like(self.layers, g, residual=self.res, outn=self.outn, **STATES[state])
        X = torch.rand(N, self.d_in, generator=g) * 2 - 1
        if self.res == "continuity_only":
            X[:, 0] = X[:, 0] * 40      # make x < 25.5 a real subset
        self.X = X

    def desc(self, **kw):
        from pinn_depthestimation_amd import NetDesc
        return NetDesc(self.d_in, self.d_out, self.L, self.W, self.gc, **kw)

    def spec(self, **kw):
        from pinn_depthestimation_amd import ResidualSpec
        return ResidualSpec.from_names(self.res, self.inn, self.gc, self.outn, **kw)

    def term_scale(self):
        if self.res == "continuity_only":
            return torch.tensor([1.0 / self.N, 1.0 / float((self.X[:, 0] < 25.5).sum()), 0.0])
        return torch.full((3 if self.res != "continuity_ftemp" else 1,), 1.0 / self.N)


def oracle_loss_grad(case, params=None, dtype=torch.float64):
    """(loss, flat gradient) of the case's residual on the CPU oracle in `dtype`, at `params` (default: the case's)."""
    from tests.golden_util import oracle_loss_and_grad
    loss, grad = oracle_loss_and_grad(case.params if params is None else params, case.X, case.res, case.inn, case.outn, case.gc, dtype)
    return float(loss), grad.double()


_REFERENCE = {}


def reference(name, state, N=N_POINTS):
    """(Case, l64, g64, l32, g32), computed once per process and shared: callers leave it unchanged."""
    key = (name, state, N)
    if key not in _REFERENCE:
        c = Case(name, state, N)
        l64, g64 = oracle_loss_grad(c, dtype=torch.float64)
        l32, g32 = oracle_loss_grad(c, dtype=torch.float32)
        _REFERENCE[key] = (c, l64, g64, l32, g32)
    return _REFERENCE[key]


def loss_bound(l64, l32):
    """tests/test_engine_gpu.py's rule for a loss: max(2e-6, 4 x the oracle's own fp32 noise), relative."""
    return max(2e-6, 4 * abs(l32 - l64) / abs(l64))


# (case, state) pairs of the loss + gradient family; the saturating state where the net has at most 3 hidden layers
FUSED_CASES = ["ns_8x64", "pe_8x64", "pe_10x10", "ns_3x12", "cf_3x32", "ns_5in", "cf_40x20", "co_3x64", "ns_out_first_3x12"]
WIDE_CASES = ["ns_3x128", "cf_2x256", "co_2x100"]
LOSS_GRAD = [(n, s) for n in FUSED_CASES + WIDE_CASES for s in STATES if s == "biased" or CASES[n][2] <= SATURATING_MAX_HIDDEN]


# ---- parameter mutants: what a kernel that mis-reads hidden biases would compute ------------------------------------------
def mutants(params):
    """{name: parameters} of four mis-readings of the hidden biases: all dropped, all rolled by one unit, the last hidden
    layer's dropped, one unit's (the last unit of the middle hidden layer) dropped."""
    n_hidden = len(params) // 2 - 1

    def edit(fn):
        q = [p.clone() for p in params]
        fn(q)
        return q

    def drop_all(q):
        for i in range(n_hidden): q[2 * i + 1].zero_()

    def roll_all(q):
        for i in range(n_hidden): q[2 * i + 1] = torch.roll(q[2 * i + 1], 1)

    def drop_last(q):
        q[2 * (n_hidden - 1) + 1].zero_()

    def drop_unit(q):
        q[2 * (n_hidden // 2) + 1][-1] = 0.0
    return {"dropped": edit(drop_all), "rolled": edit(roll_all), "last layer dropped": edit(drop_last), "one unit dropped": edit(drop_unit)}


# ---- more references for the GPU module (all on the CPU, none of them the code under test) --------------------------------
def roles(case):
    """(X columns of the residual's direction roles, Y columns of its output roles)."""
    from pinn_depthestimation_amd.engine import RESIDUAL_ROLES
    _, out_roles, dir_roles = RESIDUAL_ROLES[case.res]
    return [case.inn.index(r) for r in dir_roles], [case.outn.index(r) for r in out_roles]


def oracle_total(case, dtype, params=None, X=None, n_res=None, T=None, cols=(), weights=(), masks=None, p=0.0, init_type="xavier"):
    """(loss, flat gradient) in `dtype` of residual_loss on the first n_res rows of X (default: all) plus, with T, the
    fidelity loss sum_k w_k mean((T_k - Y_k)^2) on the rows AFTER n_res (n_res = None with T: on all rows, the one-pass
    request).  masks / p: the dropout masks handed to the oracle."""
    X = (case.X if X is None else X).to(dtype)
    q = [t.detach().to(dtype).clone().requires_grad_(True) for t in (case.params if params is None else params)]
    in_roles, out_roles = roles(case)
    Xr = X if n_res is None else X[:n_res]
    loss = O.residual_loss(q, Xr, case.res, in_roles, out_roles, case.gc, init_type,
                           None if masks is None else [m.to(dtype) for m in masks], p)
    if T is not None:
        Xf = X if n_res is None else X[n_res:]
        loss = loss + O.fidelity_loss(q, Xf, T.to(dtype), list(cols), list(weights), init_type)
    return float(loss.detach()), O.flat_grad(loss, q).double()


def oracle_fields(case, dtype, params=None, init_type="xavier"):
    """(n_fields, N) signed residual fields of the oracle in `dtype`: (fc, fm_x, fm_y) / (fc, fx, fy) / (fc, h - 0.75 where
    x < 25.5)."""
    cols = O.split_columns(case.X.to(dtype), case.gc)
    Y = O.mlp_forward([t.to(dtype) for t in (case.params if params is None else params)], torch.cat(cols, -1), init_type)
    in_roles, out_roles = roles(case)
    ins, outs = [cols[i] for i in in_roles], [Y[:, o:o + 1] for o in out_roles]
    if case.res == "Navier_Stokes":
        f = O.navier_stokes_fields(*ins, *outs)
    elif case.res == "physics_equation":
        f = O.physics_equation_fields(*ins, *outs)
    else:
        fc = O.continuity_fields(*ins, *outs)
        on = (ins[0] < 25.5) if case.res == "continuity_only" else torch.zeros_like(fc, dtype=torch.bool)
        f = (fc, torch.where(on, outs[0] - 0.75, torch.zeros_like(fc)))
    return torch.cat([t.detach() for t in f], 1).T.contiguous().double()


def jets(params, X, grad_cols, dtype, init_type="xavier", second=False):
    """(parameters with requires_grad, Y (N, d_out), dY (k, N, d_out)[, d2Y (pairs, N, d_out), pairs (i <= j) row-major]) by
    nested torch.autograd.grad in `dtype`, kept differentiable."""
    q = [t.detach().to(dtype).clone().requires_grad_(True) for t in params]
    cols = [X[:, i:i + 1].detach().to(dtype).clone().requires_grad_(True) for i in range(X.shape[1])]
    Y = O.mlp_forward(q, torch.cat(cols, -1), init_type)

    def d(a, b):
        r = torch.autograd.grad(a.sum(), b, create_graph=True, allow_unused=True)[0]
        return torch.zeros_like(b) if r is None else r

    d_out, k = Y.shape[1], len(grad_cols)
    dY = torch.stack([torch.cat([d(Y[:, c:c + 1], cols[j]) for c in range(d_out)], 1) for j in grad_cols])
    if not second:
        return q, Y, dY
    d2Y = torch.stack([torch.cat([d(dY[i][:, c:c + 1], cols[grad_cols[j]]) for c in range(d_out)], 1)
                       for i in range(k) for j in range(i, k)])
    return q, Y, dY, d2Y


def jet_adjoint_grad(params, X, grad_cols, gY, gdY, dtype, init_type="xavier"):
    """Flat gradient of sum(gY * Y) + sum(gdY * dY) by torch autograd in `dtype`."""
    q, Y, dY = jets(params, X, grad_cols, dtype, init_type)
    return O.flat_grad((gY.to(dtype) * Y).sum() + (gdY.to(dtype) * dY).sum(), q).double()


def abs_bound(ref64, floor=2e-6):
    """tests/test_engine_gpu.py's bound for forward values and jets: floor * max(1, max|ref|)."""
    return floor * max(1.0, float(ref64.abs().max()))


def residual_loss_fn(case):
    """params -> the case's residual loss on its points in float64 (for O.adam_trajectory)."""
    in_roles, out_roles = roles(case)
    return lambda q: O.residual_loss(q, case.X.double(), case.res, in_roles, out_roles, case.gc)


# ---- ensembles: every member its own draw ---------------------------------------------------------------------------------
ENSEMBLE = {
    # name: case, fidelity columns, collocation points, fidelity points (None: both terms on every point)  [test_ensemble_gpu.py]
    "pe10x10_split": ("pe_10x10", (0, 1, 2, 3, 4, 5), 243, 12),
    "ns8x64_res_only": ("ns_8x64", (), 243, 0),
    "co40x20_both": ("co_40x20", (0, 1), 100, None),
}
ENSEMBLE_M = 3
_ENSEMBLE = {}


def ensemble_reference(name):
    """(Case, members [M parameter lists, each its own trained_like draw], T or None, [(l64, g64, l32, g32) per member]),
    computed once per process and shared: callers leave it unchanged."""
    if name not in _ENSEMBLE:
        cname, fid, n_r, n_f = ENSEMBLE[name]
        c = Case(cname, "biased", N=n_r + (n_f or 0), seed=77)
        g = torch.Generator().manual_seed(78)
        members = [trained_like(c.layers, g, residual=c.res, outn=c.outn) for _ in range(ENSEMBLE_M)]
        T = torch.rand(n_r if n_f is None else n_f, len(fid), generator=g) if fid else None
        refs = []
        for pm in members:
            kw = dict(params=pm, n_res=None if n_f is None or n_f == 0 else n_r, T=T, cols=fid, weights=[1.0] * len(fid))
            refs.append(oracle_total(c, torch.float64, **kw) + oracle_total(c, torch.float32, **kw))
        _ENSEMBLE[name] = (c, members, T, refs)
    return _ENSEMBLE[name]

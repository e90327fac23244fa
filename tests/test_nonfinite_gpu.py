"""Non-finite values through every kernel family (tests/nonfinite_util.py has the networks, the sites and the reference).

One NaN — in X at point 0, 16 or N - 1 (the point tail lanes are clamped to), in an input column that is not differentiated,
in a hidden weight, a hidden bias or a target — must make the loss sums and the gradient NaN exactly where
oracle/pinn_oracle.py in fp32 has a NaN on the same data, leave every sum the oracle leaves finite at the very bits of the
unpoisoned call on the same engine, and, in the per-point outputs, own exactly its row: every other row keeps the bits of
the unpoisoned call.  tests/test_nonfinite_cpu.py asserts what this presumes about the oracle."""
import math

import pytest
import torch

from oracle import pinn_oracle as O
from tests import nonfinite_util as U

pytestmark = pytest.mark.gpu

LOSS_CASES = [(name, e) for name in U.NETS for e in U.NETS[name][-1]]
VARIANTS = [("pe_3x10", "corrected"), ("ns_3x48", "weighted"), ("pe_3x10", "coef"), ("ns_3x20_5in", "sine")]
_ENGINES = {}


def _engine(n, engine, variant="plain"):
    from pinn_depthestimation_amd import Engine, _lib as L
    key = (n.name, engine, variant)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(n.desc(engine, activation=L.ACT_SIN_TANH if variant == "sine" else L.ACT_TANH), "cuda:0")
    return _ENGINES[key]


def _loss(n, engine, split, site, variant="plain", value=math.nan):
    """(term sums, column sums or None, gradient) of the engine on the data poisoned at `site`, on the CPU."""
    params, X, T = U.poisoned(n, site, value)
    eng = _engine(n, engine, variant)
    flat = O.flatten(params).cuda()
    grad = torch.zeros_like(flat)
    spec = n.spec(corrected=variant == "corrected")
    ts_scale = torch.tensor(U.TERM_SCALE, device="cuda")
    cs = None
    if split:
        ts, cs = eng.residual_mse_split_loss_grad(spec, ts_scale, T.cuda(), U.FID_COLS, torch.tensor(U.COL_SCALE, device="cuda"),
                                                  flat, X.cuda(), U.N_RES, grad)
        cs = cs.cpu()
    else:
        Xd = X[:U.N_RES].contiguous().cuda()
        if variant == "weighted":
            ts = eng.residual_weighted_loss_grad(spec, U.point_weights().cuda(), ts_scale, flat, Xd, grad)
        elif variant == "coef":
            ts = eng.residual_coef_loss_grad(spec, torch.tensor([U.COEF[n.res]], device="cuda"), ts_scale, flat, Xd, grad)
        else:
            ts = eng.residual_loss_grad(spec, ts_scale, flat, Xd, grad)
    torch.cuda.synchronize()
    return ts.cpu(), cs, grad.cpu()


def _check_loss(name, engine, split, variant="plain"):
    n = U.net(name)
    ts0, cs0, g0 = _loss(n, engine, split, None, variant)
    assert torch.isfinite(ts0).all() and torch.isfinite(g0).all() and (cs0 is None or torch.isfinite(cs0).all())
    bad = []
    for site in n.sites(split):
        rts, rcs, rg = U.reference_loss(name, site, split, variant)
        ts, cs, g = _loss(n, engine, split, site, variant)
        m = U.nan_mismatch(ts, rts)
        if m: bad.append((site, "term sums: NaN pattern differs from the oracle's", m, ts.tolist(), rts.tolist()))
        fin = ~torch.isnan(rts)
        d = U.bits_differ(ts[fin], ts0[fin])
        if d: bad.append((site, "finite term sums differ from the unpoisoned call's", d, ts.tolist(), ts0.tolist()))
        if split:
            m = U.nan_mismatch(cs, rcs)
            if m: bad.append((site, "column sums: NaN pattern differs from the oracle's", m, cs.tolist(), rcs.tolist()))
            fin = ~torch.isnan(rcs)
            d = U.bits_differ(cs[fin], cs0[fin])
            if d: bad.append((site, "finite column sums differ from the unpoisoned call's", d, cs.tolist(), cs0.tolist()))
        m = U.nan_mismatch(g, rg)
        if m: bad.append((site, f"gradient: {len(m)} of {g.numel()} entries differ in NaN-ness from the oracle's", m[:12],
                          [float(g[i]) for i in m[:12]], [float(rg[i]) for i in m[:12]]))
    assert not bad, (name, engine, "split" if split else "residual", variant, bad)


@pytest.mark.parametrize("name,engine", LOSS_CASES)
def test_nan_reaches_sums_and_gradient_split(name, engine):
    """The split request (37 residual rows + 21 fidelity rows in one call), every site."""
    _check_loss(name, engine, True)


@pytest.mark.parametrize("name,engine", LOSS_CASES)
def test_nan_reaches_sums_and_gradient_residual(name, engine):
    """The residual request on the 37 collocation points alone: the poisoned point N - 1 is the one tail lanes are clamped to."""
    _check_loss(name, engine, False)


@pytest.mark.parametrize("name,variant", VARIANTS)
def test_nan_reaches_sums_and_gradient_tile_variants(name, variant):
    """The tile kernel's other instances: corrected radiation stress, point weights, closure coefficient, sine first layer."""
    _check_loss(name, "tile", False, variant)


def _points(n, engine, site, value=math.nan, variant="plain"):
    params, X, _ = U.poisoned(n, site, value)
    eng = _engine(n, engine, variant)
    flat, Xd = O.flatten(params).cuda(), X[:U.N_RES].contiguous().cuda()
    Y = eng.forward(flat, Xd)
    Yj, dY = eng.forward_jet(flat, Xd)
    F = eng.residual_fields(n.spec(), flat, Xd)
    torch.cuda.synchronize()
    return Y.cpu(), Yj.cpu(), dY.cpu(), F.cpu()


@pytest.mark.parametrize("name,engine", LOSS_CASES)
def test_nan_stays_in_its_row(name, engine):
    """pinn_forward, pinn_forward_jet, pinn_residual_fields: the poisoned point's row is NaN where the oracle's is, every other
    row is the unpoisoned call's bit for bit; a poisoned parameter poisons what the oracle says it does."""
    n = U.net(name)
    clean = _points(n, engine, None)
    assert all(torch.isfinite(t).all() for t in clean)
    bad = []
    for site in n.sites(False):
        rY, rdY, rF = U.reference_points(name, site)
        got = _points(n, engine, site)
        r = U.row_of(site)
        # row-major views (N first) of the four outputs and of the oracle's
        views = [("forward Y", got[0], clean[0], rY), ("jet Y", got[1], clean[1], rY),
                 ("jet dY", got[2].permute(1, 0, 2), clean[2].permute(1, 0, 2), rdY.permute(1, 0, 2)),
                 ("fields", got[3].T, clean[3].T, rF.T)]
        for what, g, c, ref in views:
            g, c, ref = g.contiguous(), c.contiguous(), ref.contiguous()
            rows = [r] if r is not None else list(range(U.N_RES))
            for i in rows:
                m = U.nan_mismatch(g[i], ref[i])
                if m: bad.append((site, what, f"row {i}: NaN pattern differs from the oracle's", g[i].reshape(-1).tolist(), ref[i].reshape(-1).tolist())); break
            if r is not None:
                keep = [i for i in range(U.N_RES) if i != r]
                d = U.bits_differ(g[keep], c[keep])
                if d: bad.append((site, what, f"{len(d)} entries of OTHER rows differ from the unpoisoned call's", d[:8]))
    assert not bad, (name, engine, bad)


@pytest.mark.parametrize("name,engine", LOSS_CASES)
def test_inf_row_stays_finite(name, engine):
    """One +inf per engine, at X[16] in a differentiated column, on the per-point outputs: the oracle's row is finite (tanh
    saturates), the engine's must be finite and within the forward tolerance of tests/test_engine_gpu.py (2e-6 times
    max(1, largest reference entry); bf16 mode: tests/test_wide_gpu.py's 5e-2) of the fp64 oracle — Y, the jet's Y and dY, and
    the residual fields alike (the tile kernel's field instances are kernels of their own).  The inf-times-zero pattern of the layer-0 gradient under that +inf is
    printed, not asserted (DESIGN.md 4.6 has the table).

    The MFMA kernels with a padded hidden width (10 -> 16, 20 -> 32, 48 -> 64) hand X to layer 0 through finite_input
    (residuals.h): a padded unit's zero weights would otherwise give 0 * inf = NaN in layer 0 and 0 * NaN in every real unit of
    layer 1."""
    n = U.net(name)
    bad = []
    tol = 5e-2 if engine == "wide_bf16" else 2e-6
    rY, rdY, rF = U.reference_points(name, "x16", math.inf, torch.float64)
    Y, Yj, dY, F = _points(n, engine, "x16", math.inf)
    for what, g, ref in (("forward Y", Y, rY), ("jet Y", Yj, rY), ("jet dY", dY, rdY), ("fields", F, rF)):
        if not torch.isfinite(g).all():
            bad.append(("+inf at x16", what, "not finite", torch.nonzero(~torch.isfinite(g)).tolist()[:8]))
        else:
            e = float((g.double() - ref).abs().max())
            if not e < tol * max(1.0, float(ref.abs().max())):
                bad.append(("+inf at x16", what, f"error {e:.3e} against the fp64 oracle"))
    _, _, g = _loss(n, engine, False, "x16", value=math.inf)
    params, X, T = U.poisoned(n, "x16", math.inf)
    og = U.oracle_loss(n, params, X[:U.N_RES])[2]
    nw0 = n.layers[0] * n.layers[1]
    print(f"+inf at X[16, {n.gc[-1]}], {name} on {engine}: NaN entries of the W_0 gradient {int(torch.isnan(g[:nw0]).sum())} of {nw0} "
          f"(fp32 oracle: {int(torch.isnan(og[:nw0]).sum())}), of the whole gradient {int(torch.isnan(g).sum())} of {g.numel()} "
          f"(oracle: {int(torch.isnan(og).sum())})")
    assert not bad, (name, engine, bad)


@pytest.mark.parametrize("name", ["ns_3x20_5in"])
def test_nan_stays_in_its_row_sine(name):
    """The sine first layer's forward and jet on the tile kernel, the same way (its residual fields run on the generic engine)."""
    n = U.net(name)
    params0, X0, _ = U.poisoned(n, None)
    eng = _engine(n, "tile", "sine")

    def run(site):
        params, X, _ = U.poisoned(n, site)
        flat, Xd = O.flatten(params).cuda(), X[:U.N_RES].contiguous().cuda()
        Y = eng.forward(flat, Xd)
        Yj, dY = eng.forward_jet(flat, Xd)
        return Y.cpu(), Yj.cpu(), dY.cpu().permute(1, 0, 2).contiguous()
    clean = run(None)
    assert all(torch.isfinite(t).all() for t in clean)
    for site in U.X_SITES:
        rY, rdY, _ = U.reference_points(name, site, variant="sine")
        got, r = run(site), U.row_of(site)
        keep = [i for i in range(U.N_RES) if i != r]
        for g, c, ref in zip(got, clean, (rY, rY, rdY.permute(1, 0, 2).contiguous())):
            assert not U.nan_mismatch(g[r], ref[r]), (site, g[r], ref[r])
            assert not U.bits_differ(g[keep], c[keep]), site

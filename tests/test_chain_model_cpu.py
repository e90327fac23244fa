"""The fp64 rounding model of bf16 mode (tests/chain_model_util.py), checked without a GPU:

  * with every rounding switched off the hand-written forward and reverse sweeps equal the fp64 oracle (loss terms and
    gradient through the real network by torch autograd) to 1e-10;
  * every case of the table and every sweep draw that is not skipped has finite references and a bound (max(fp32 floor,
    4 x emulation noise)) of at most 1e-3 on every term sum and gradient block; at most 10 % of the draws are skipped;
  * the cases reach every dispatch branch of run_w (a predicate restating its conditions, at 256 CUs);
  * every mutant — a plausible mis-reading of the kernels applied to the model — is rejected by at least one case under
    that case's bounds; the weakest of the best rejections is printed.

Measured here (mutant's distance from the model / the case's bound, best quantity of the best case): lo dropped in a hidden
layer's forward 3 500, in a reverse product 142, in the output layer's forward 10 000; forward 1 - a^2 from the rounded a
1 760; reverse 1 - a^2 from the unrounded a 138; zbar unrounded in the weight gradient 87 (the weakest); abar_L unrounded 167;
one tangent unrounded 3 100; point 7 of 16 on the previous layer's weights 11 900; a hidden bias block shifted by one unit
459 000.  No mutant is missed.  Sweep draws skipped for a condition of their reference: 7022 (2 x 129 at one point: bounds up
to 9.5e-3, above the cap).
"""
import pytest
import torch

from oracle import pinn_oracle as O
from tests import chain_model_util as M

CUS = M.MI355X_CUS
SMALL = [c for c in M.TABLE if c.n[0] == 0]


def oracle_through_network(c, params, X, T, rq):
    """(sums, csums, flat gradient) in fp64 through the real network: the oracle's residual functions and autograd."""
    from pinn_depthestimation_amd.engine import RESIDUAL_ROLES
    dt = torch.float64
    q = [p.detach().to(dt).clone().requires_grad_(True) for p in params]
    N, n_res = X.shape[0], rq["n_res"]
    total, sums, csums = torch.zeros((), dtype=dt), torch.zeros(0, dtype=dt), torch.zeros(0, dtype=dt)
    if rq["kind"] != "mse":
        _, out_roles, dir_roles = RESIDUAL_ROLES[c.res]
        cols = O.split_columns(X[:n_res].to(dt), c.gc)
        Y = O.mlp_forward(q, torch.cat(cols, -1))
        ins = [cols[c.inn.index(r)] for r in dir_roles]
        outs = [Y[:, c.outn.index(r):c.outn.index(r) + 1] for r in out_roles]
        if c.res == "Navier_Stokes":
            f = list(O.navier_stokes_fields(*ins, *outs))
        elif c.res == "physics_equation":
            f = list(O.physics_equation_fields(*ins, *outs))
        else:
            f = [O.continuity_fields(*ins, *outs)]
        s = [(x ** 2).sum() for x in f]
        if c.res == "continuity_only":
            on = ins[0] < 25.5
            s += [(torch.where(on, outs[0] - 0.75, torch.zeros_like(outs[0])) ** 2).sum(), on.sum().to(dt)]
        sums = torch.stack(s)
        total = total + (rq["scale"].to(dt) * sums).sum()
    if rq["kind"] in ("mse", "split", "onepass"):
        Xf = X[n_res:] if rq["kind"] == "split" else X
        Tt = T[: N - n_res] if rq["kind"] == "split" else T
        Yf = O.mlp_forward(q, Xf.to(dt))
        csums = torch.stack([((Tt[:, j].to(dt) - Yf[:, o]) ** 2).sum() for j, o in enumerate(rq["cols"])])
        total = total + (rq["cscale"].to(dt) * csums).sum()
    return sums.detach(), csums.detach(), O.flat_grad(total, q).double()


@pytest.mark.parametrize("name,kind", [("L1_ns_w128_n70", "residual"), ("L1_pe_w200_n17", "mse"), ("L2_co_w100_n243", "split"),
                                       ("L3_ns_w129_n70", "residual"), ("L3_pe_w128_n1000", "residual"), ("L3_pe_w128_n1000", "split"),
                                       ("L3_ns4_w100_n1000", "residual"), ("L4_cf_w200_n1000", "mse"), ("L6_ns_w128_damped", "residual")])
def test_model_without_rounding_is_the_fp64_oracle(name, kind):
    c = M.TABLE_BY_NAME[name]
    params, X, T = c.data(CUS)
    rq = c.request(kind, CUS)
    got = M.run(c, params, X, T, rq, rounding=False)
    sums, csums, grad = oracle_through_network(c, params, X, T, rq)
    worst = 0.0
    for a, b in ((got["sums"], sums), (got["csums"], csums)):
        for x, y in zip(a, b):
            worst = max(worst, abs(float(x) - float(y)) / max(abs(float(y)), 1e-300))
    eg = M.distances(c, dict(grad=got["grad"]), dict(grad=grad))
    print(f"CHAIN MODEL identity | {name} {kind}: sums {worst:.1e}, worst block {max(eg.values()):.1e}")
    assert worst < 1e-10 and max(eg.values()) < 1e-10, (worst, eg)
    Yo = O.mlp_forward([p.double() for p in params], X.double())
    assert float((got["Y"] - Yo).abs().max()) < 1e-12


@pytest.mark.parametrize("c", M.TABLE, ids=lambda c: c.name)
def test_case_bounds_stay_within_the_cap(c):
    for kind in c.calls:
        model, bound, noise = M.reference(c, kind, CUS)
        for k, (_, v) in M.quantities(c, model).items():
            assert bool(torch.isfinite(v).all()), (c.name, kind, k)
        over = M.capped(c, bound)
        top = max((k for k in bound if k.startswith(("sum", "col", "W", "b"))), key=bound.get, default=None)
        print(f"CHAIN MODEL bound | {c.name} {kind} N={c.N(CUS)}: largest sum/block bound {top} {bound.get(top, 0):.1e}, "
              f"largest jet bound {max((b for k, b in bound.items() if k[0] in 'Ydf'), default=0):.1e}")
        assert not over, (c.name, kind, over)


def test_sweep_draws_stay_within_the_cap_and_few_are_skipped():
    skipped = {}
    for seed in M.SWEEP_SEEDS:
        c = M.draw(seed)
        kind = c.calls[0]
        why = M.cancelling(c, kind, CUS)
        if why is None:
            _, bound, _ = M.reference(c, kind, CUS)
            over = M.capped(c, bound)
            if over:
                why = "bound above the cap: " + ", ".join(f"{k} {v:.1e}" for k, v in over.items())
        if why:
            skipped[seed] = why
    print("CHAIN MODEL sweep | skipped:", skipped or "none")
    assert len(skipped) <= len(M.SWEEP_SEEDS) // 10, skipped


def test_every_dispatch_branch_is_reached():
    seen = {k: set() for k in M.ALL_BRANCHES}
    rows = []
    for c in M.TABLE + [M.draw(s) for s in M.SWEEP_SEEDS]:
        for kind in c.calls:
            b = M.branches(c, kind, CUS)
            rows.append((c.name, kind, b))
            for k, v in b.items():
                seen[k].add(v)
    for name, kind, b in rows[:len(M.TABLE) * 2]:
        print(f"CHAIN MODEL census | {name} {kind}: {b}")
    assert seen == M.ALL_BRANCHES, {k: M.ALL_BRANCHES[k] - seen[k] for k in seen}
    # the combinations the issue names: several batches with one hidden matrix, with the wide first layer, at every K1 and NTW
    def has(**kw):
        return any(all(b[k] == v for k, v in kw.items()) for _, _, b in rows)
    for kw in (dict(batches="several", nh="1"), dict(batches="several", first="wide"), dict(batches="several", K1=1),
               dict(batches="several", K1=3), dict(batches="several", K1=4), dict(batches="several", NTW=8),
               dict(batches="several", NTW=16), dict(batches="several", last_bwd="wide"), dict(nh="0", last_bwd="wide")):
        assert has(**kw), kw


def test_noise_against_depth():
    """The table of DESIGN.md section 4.4: emulation noise of the largest term sum / gradient block against depth, width 128,
    4 000 points, gain 1 (and 0.65 at depth 6): why the model is used at depth <= 4 and damped at depth 6."""
    for L, gain in ((1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (6, 1.0), (6, 0.65), (12, 1.0)):
        c = M.Case(f"depth{L}_{gain}", "ns", L, 128, (0, 4000), gain=gain)
        _, bound, noise = M.reference(c, "residual", CUS)
        s = max(v for k, v in noise.items() if k.startswith("sum"))
        b = max(v for k, v in noise.items() if k[0] in "Wb")
        print(f"CHAIN MODEL depth | L={L} gain={gain}: noise sums {s:.1e} blocks {b:.1e}")
        if L <= 4 or (L == 6 and gain == 0.65):
            assert 4 * max(s, b) <= M.CAP


def test_every_mutant_is_rejected():
    best = {}
    for c in SMALL:
        kind = "residual" if "residual" in c.calls else c.calls[0]
        params, X, T = c.data(CUS)
        rq = c.request(kind, CUS)
        model, bound, _ = M.reference(c, kind, CUS)
        for m in M.MUTANTS:
            r = M.ratios(c, M.run(c, params, X, T, rq, mutant=m), model, bound)
            k = max(r, key=r.get)
            if r[k] > best.get(m, (0, None, None))[0]:
                best[m] = (r[k], c.name, k)
    for m in M.MUTANTS:
        print(f"CHAIN MODEL mutant | {m}: best rejection {best[m][0]:.1f} x bound ({best[m][1]}, {best[m][2]})")
    weakest = min(best, key=lambda m: best[m][0])
    print(f"CHAIN MODEL mutant | weakest: {weakest} at {best[weakest][0]:.1f} x bound")
    missed = [m for m in M.MUTANTS if not best[m][0] > 1.0]
    assert not missed, {m: best[m] for m in missed}

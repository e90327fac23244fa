"""What tests/test_nonfinite_gpu.py presumes about its reference, asserted: on oracle/pinn_oracle.py in fp32 a NaN in X or in
a parameter makes EVERY gradient entry and every sum that includes the point NaN, a NaN in a target makes only its column
sum and the gradient NaN, and in the per-point outputs a poisoned point owns exactly its row.  The GPU module's
expectations ("NaN exactly where the oracle's is") are therefore not vacuous."""
import math

import pytest
import torch

from tests import nonfinite_util as U


@pytest.mark.parametrize("name", list(U.NETS))
@pytest.mark.parametrize("split", [False, True], ids=["residual", "split"])
def test_oracle_loss_patterns(name, split):
    n = U.net(name)
    ts0, cs0, g0 = U.reference_loss(name, None, split)
    assert torch.isfinite(ts0).all() and torch.isfinite(g0).all() and (cs0 is None or torch.isfinite(cs0).all())
    assert float(ts0.min()) > 0                                          # every term takes part
    for site in n.sites(split):
        ts, cs, g = U.reference_loss(name, site, split)
        hidden = sum(n.layers[i] * n.layers[i + 1] + n.layers[i + 1] for i in range(n.L))
        if site in U.SPLIT_ONLY:
            # only the fidelity columns see the NaN: the residual's sums are the clean ones, every hidden parameter's gradient
            # is NaN, and in the output layer what belongs to the other columns alone stays finite
            assert torch.equal(ts, ts0) and torch.isnan(g[:hidden]).all() and torch.isfinite(g[hidden:]).any(), site
            if site == "t":
                assert torch.equal(cs[:1], cs0[:1]) and math.isnan(float(cs[1])), site
            else:
                assert torch.isnan(cs).all(), site
        else:
            assert torch.isnan(ts).all() and torch.isnan(g).all(), site
            if split:
                assert torch.isnan(cs).all() if site in U.PARAM_SITES else torch.equal(cs, cs0), site


@pytest.mark.parametrize("name,variant", [("pe_3x10", "corrected"), ("ns_3x48", "weighted"), ("pe_3x10", "coef"), ("ns_3x20_5in", "sine")])
def test_oracle_variant_patterns(name, variant):
    n = U.net(name)
    ts0, _, g0 = U.reference_loss(name, None, False, variant)
    assert torch.isfinite(ts0).all() and torch.isfinite(g0).all()
    for site in n.sites(False):
        ts, _, g = U.reference_loss(name, site, False, variant)
        # (the coefficient formula leaves physics_equation's Hrms and k out: their output rows are unused, gradient 0)
        assert torch.isnan(ts).all() and torch.isnan(g[g0 != 0]).all(), site


@pytest.mark.parametrize("name", list(U.NETS))
def test_oracle_point_patterns(name):
    n = U.net(name)
    clean = U.reference_points(name, None)
    assert all(torch.isfinite(t).all() for t in clean)
    for site in n.sites(False):
        Y, dY, F = U.reference_points(name, site)
        r = U.row_of(site)
        if r is None:
            assert torch.isnan(Y).all() and torch.isnan(dY).all() and torch.isnan(F).all(), site
            continue
        rows = torch.arange(U.N_RES) != r
        assert torch.isnan(Y[r]).all() and torch.isnan(dY[:, r]).all() and torch.isnan(F[:, r]).all(), site
        assert torch.isfinite(Y[rows]).all() and torch.isfinite(dY[:, rows]).all() and torch.isfinite(F[:, rows]).all(), site
    # +inf in a differentiated column: tanh saturates, the row stays finite (fp64: what the engines are held to)
    Y, dY, F = U.reference_points(name, "x16", math.inf, torch.float64)
    assert torch.isfinite(Y).all() and torch.isfinite(dY).all() and torch.isfinite(F).all()

"""pinn_jet_backward on the MFMA tile kernel (k_fused with the external-adjoint epilogue): the parameter gradient of
ANY loss written with compute_gradient.  Checker: oracle/pinn_oracle.py in float64 (torch autograd over the oracle's
forward), the way tests/test_sweep_gpu.py checks the generic engine.  Bars: rel_l2 < 2e-5 for the flat gradient, the
project's bar for this quantity (tests/test_engine_gpu.py, tests/test_sweep_gpu.py, tests/test_fullsize_gpu.py)."""
import random

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, PinnError
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ACT_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH,
                                           ENGINE_FUSED_COOP, ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE)

pytestmark = pytest.mark.gpu

TOL = 2e-5


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def init_of(desc):
    return "kaiming" if desc.activation == ACT_LEAKY_RELU else "xavier"


def make(desc, N, seed):
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(desc.layers, init_of(desc), g)
    X = torch.rand(N, desc.d_in, generator=g) * 2 - 1
    gY = torch.randn(N, desc.d_out, generator=g)
    gdY = torch.randn(max(desc.k, 1), N, desc.d_out, generator=g)[:desc.k]
    return params, X, gY, gdY


def oracle_grad(desc, params, X, gY, gdY):
    """float64 d/dtheta [sum(gY * Y) + sum(gdY * dY)] by torch autograd over the oracle's network."""
    p64 = [p.double().clone().requires_grad_(True) for p in params]
    cols = O.split_columns(X.double(), desc.grad_cols)
    Y = O.mlp_forward(p64, torch.cat(cols, -1), init_of(desc))
    obj = 0.0
    if gY is not None:
        obj = obj + (gY.double() * Y).sum()
    if gdY is not None:
        dY = torch.stack([torch.cat([O.compute_gradient(Y[:, c:c + 1], cols[j]) for c in range(desc.d_out)], 1)
                          for j in desc.grad_cols])
        obj = obj + (gdY.double() * dY).sum()
    return O.flat_grad(obj, p64)


def run(desc, engine, params, X, gY, gdY, grad=None):
    eng = Engine(desc.with_(engine=engine))
    grad = torch.zeros(desc.n_params, device="cuda") if grad is None else grad
    eng.jet_backward(O.flatten(params).cuda(), X.cuda(), None if gY is None else gY.cuda(),
                     None if gdY is None else gdY.cuda(), grad)
    torch.cuda.synchronize()
    return grad


CASES = {
    # name: (descriptor, N)
    "w16_pe_10x10": (NetDesc(2, 6, 10, 10, (0, 1)), 700),
    "w32_ns_5in": (NetDesc(5, 4, 3, 20, (0, 1, 2)), 200),
    "w64_ns_8x64": (NetDesc(3, 4, 8, 64, (0, 1, 2)), 1000),
    "w64_k2_dout7": (NetDesc(3, 7, 2, 48, (2, 0)), 333),
    "w64_dout13": (NetDesc(4, 13, 3, 33, (0, 1, 3)), 333),
    "w32_din16_dout5": (NetDesc(16, 5, 2, 30, (3, 9, 15)), 150),
    "w16_din16_dout16": (NetDesc(16, 16, 2, 16, (0, 15)), 97),
    "single_hidden_w10": (NetDesc(2, 6, 1, 10, (0, 1)), 333),
    "single_hidden_w64": (NetDesc(3, 4, 1, 64, (0, 1, 2)), 333),
    "no_lds_40x20": (NetDesc(2, 3, 40, 20, (0, 1)), 333),
    "no_lds_40x20_k3": (NetDesc(3, 3, 40, 20, (0, 1, 2)), 120),
    "leaky_w16": (NetDesc(2, 3, 3, 16, (0, 1), ACT_LEAKY_RELU), 333),
    "leaky_w32_k3": (NetDesc(3, 7, 4, 32, (0, 1, 2), ACT_LEAKY_RELU), 500),
    "leaky_w64": (NetDesc(2, 6, 3, 64, (0, 1), ACT_LEAKY_RELU), 333),
    "leaky_no_lds": (NetDesc(2, 3, 40, 20, (0, 1), ACT_LEAKY_RELU), 100),
    "n_below_a_tile": (NetDesc(3, 4, 8, 64, (0, 1, 2)), 7),
    "one_point_w16": (NetDesc(2, 6, 10, 10, (0, 1)), 1),
    "n_tile_plus_one": (NetDesc(2, 3, 4, 20, (0, 1)), 17),
    "plain_net_k0": (NetDesc(3, 4, 4, 48, ()), 333),
    "plain_net_k0_w16": (NetDesc(2, 5, 3, 12, ()), 50),
}


@pytest.mark.parametrize("mode", ["both", "gY", "gdY"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_against_the_fp64_oracle(name, mode):
    desc, N = CASES[name]
    if desc.k == 0 and mode != "gY":
        return          # a network without differentiated inputs has no gdY: its one mode is "gY"
    params, X, gY, gdY = make(desc, N, seed=41)
    gY = None if mode == "gdY" else gY
    gdY = None if mode == "gY" else gdY
    ref = oracle_grad(desc, params, X, gY, gdY)
    got = run(desc, ENGINE_FUSED, params, X, gY, gdY)
    rel = rel_l2(got, ref)
    print(f"{name} {mode}: rel_l2 {rel:.2e}")
    assert rel < TOL, (name, mode, rel)


def draw_served_net(seed):
    """draw_net of tests/test_sweep_gpu.py restricted to what the MFMA path serves: width <= 64, d_in and d_out <= 16,
    0, 2 or 3 differentiated inputs."""
    r = random.Random(seed)
    d_in, d_out = r.choice([2, 3, 4, 6, 11, 16]), r.choice([1, 2, 3, 4, 5, 6, 7, 9, 13, 16])
    k = r.choice([0, 2, 2, 3, 3])
    gc = tuple(sorted(r.sample(range(d_in), min(k, d_in))))
    W = r.choice([3, 8, 10, 16, 17, 20, 24, 32, 33, 48, 50, 64])
    L = r.choice([1, 2, 3, 5, 8, 12, 30])
    N = r.choice([1, 15, 16, 100, 243, 1000, 2049, 4101])
    act = r.choice([ACT_TANH, ACT_TANH, ACT_LEAKY_RELU])
    return NetDesc(d_in, d_out, L, W, gc, act), N


@pytest.mark.parametrize("seed", range(7000, 7048))
def test_random_networks_fused_against_oracle_and_generic(seed):
    desc, N = draw_served_net(seed)
    params, X, gY, gdY = make(desc, N, seed)
    rels = []
    for with_gdY in ((True, False) if desc.k else (False,)):
        gd = gdY if with_gdY else None
        ref = oracle_grad(desc, params, X, gY, gd)
        fused = run(desc, ENGINE_FUSED, params, X, gY, gd)
        generic = run(desc, ENGINE_GENERIC, params, X, gY, gd)
        rels.append((rel_l2(fused, ref), rel_l2(fused, generic)))
    print(f"seed {seed}: {desc.d_in}->{desc.n_hidden}x{desc.width}->{desc.d_out} act={desc.activation} k={desc.k} N={N}: {rels}")
    for ro, rg in rels:
        assert ro < TOL and rg < TOL, (seed, rels)


@pytest.mark.parametrize("name", ["w64_ns_8x64", "w16_pe_10x10", "no_lds_40x20"])
def test_gradient_is_added_to_what_grad_holds(name):
    desc, N = CASES[name]
    params, X, gY, gdY = make(desc, N, seed=5)
    g0 = run(desc, ENGINE_FUSED, params, X, gY, gdY)
    pre = torch.randn(desc.n_params, generator=torch.Generator().manual_seed(6)).cuda()
    g1 = run(desc, ENGINE_FUSED, params, X, gY, gdY, grad=pre.clone())
    assert rel_l2(g1 - pre, g0) < 1e-6
    assert float((g1 - pre).abs().max()) > 0.0


REFUSED = {
    "width_100": (NetDesc(3, 4, 2, 100, (0, 1, 2)), True, "width 100"),
    "k1_with_gdY": (NetDesc(3, 4, 3, 48, (1,)), True, "k = 1"),
    "dropout": (NetDesc(3, 4, 3, 48, (0, 1, 2), dropout_p=0.25), True, "dropout"),
    "dropout_w20": (NetDesc(2, 3, 3, 20, (0, 1), dropout_p=0.25), True, "dropout"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
@pytest.mark.parametrize("fused", [ENGINE_FUSED, ENGINE_FUSED_TILE, ENGINE_FUSED_COOP, ENGINE_FUSED_BATCH])
def test_fused_refuses_what_auto_sends_to_the_generic_engine(name, fused):
    desc, with_gdY, why = REFUSED[name]
    params, X, gY, gdY = make(desc, 211, seed=8)
    with pytest.raises(PinnError, match=why):
        run(desc, fused, params, X, gY, gdY)
    auto = run(desc, ENGINE_AUTO, params, X, gY, gdY)
    generic = run(desc, ENGINE_GENERIC, params, X, gY, gdY)
    assert torch.equal(auto, generic)          # AUTO IS the generic engine here, and that engine is reproducible


def test_wide_engine_is_refused():
    desc = NetDesc(3, 4, 3, 128, (0, 1, 2))
    params, X, gY, gdY = make(desc, 211, seed=8)
    with pytest.raises(PinnError, match="wide engine"):
        run(desc, ENGINE_WIDE, params, X, gY, gdY)
    assert torch.equal(run(desc, ENGINE_AUTO, params, X, gY, gdY), run(desc, ENGINE_GENERIC, params, X, gY, gdY))


def test_engine_keyword_overrides_the_descriptor():
    desc, N = CASES["w32_ns_5in"]
    params, X, gY, gdY = make(desc, N, seed=9)
    eng = Engine(desc.with_(engine=ENGINE_GENERIC))
    flat, Xd = O.flatten(params).cuda(), X.cuda()
    g_gen = eng.jet_backward(flat, Xd, gY.cuda(), gdY.cuda(), torch.zeros(desc.n_params, device="cuda"))
    g_fus = eng.jet_backward(flat, Xd, gY.cuda(), gdY.cuda(), torch.zeros(desc.n_params, device="cuda"), engine=ENGINE_FUSED)
    ref = oracle_grad(desc, params, X, gY, gdY)
    assert rel_l2(g_gen, ref) < TOL and rel_l2(g_fus, ref) < TOL


@pytest.mark.parametrize("desc,N", [(NetDesc(2, 6, 3, 24, (0, 1)), 400), (NetDesc(3, 4, 8, 64, (0, 1, 2)), 1000)],
                         ids=["3x24_N400", "8x64_N1000"])
@pytest.mark.parametrize("fused", [ENGINE_FUSED, ENGINE_AUTO])
def test_small_requests_are_bit_reproducible(desc, N, fused):
    """One workgroup per tile and workgroup-major wave numbering: while N <= 16 x the workgroups launched, one wave adds
    to each gradient copy in program order (include/pinn_hip.h, pinn_jet_backward)."""
    params, X, gY, gdY = make(desc, N, seed=12)
    first = run(desc, fused, params, X, gY, gdY)
    for _ in range(3):
        assert torch.equal(run(desc, fused, params, X, gY, gdY), first)
    assert rel_l2(first, oracle_grad(desc, params, X, gY, gdY)) < TOL


# ---- the drop-in face: losses written with compute_gradient that are none of the four hard-wired residuals ----------

def burgers(t, x, y, h, z, u, v):
    from pinn_depthestimation_amd.physics import compute_gradient as d
    r1 = d(u, t) + u * d(u, x) + v * d(u, y)
    r2 = d(v, t) + u * d(v, x) + v * d(v, y) + 0.3 * d(h + z, y)
    return torch.mean(r1 ** 2) + torch.mean(r2 ** 2) + 0.1 * torch.mean((h - 0.5) ** 2)


def corrected_pe(x, y, *outs):
    from pinn_depthestimation_amd import physics
    return physics.physics_equation(x, y, *outs, corrected=True)


def dropin_model(layers, seed):
    from pinn_depthestimation_amd.dnn import DNN
    torch.manual_seed(seed)
    model = DNN(layers, 0.0, "xavier").to("cuda")
    if layers[-1] == 6:       # keep eta_mean + h away from 0 and k h away from 0 (1 / sinh(2 k h))
        last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.bias[4] = 0.2; last.bias[5] = 1.0; last.bias[0] = 2.0
    return model


def fp64_reference(model, Xh, loss_fn):
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in model._ordered_params()]
    cols = [Xh[:, i:i + 1].double().clone().requires_grad_(True) for i in range(Xh.shape[1])]
    pred = O.mlp_forward(p64, torch.cat(cols, -1))
    loss = loss_fn(*cols, *[pred[:, i:i + 1] for i in range(pred.shape[1])])
    return loss, O.flat_grad(loss, p64)


@pytest.mark.parametrize("case", ["corrected_pe_3x24", "corrected_pe_8x64", "burgers_4x20", "burgers_8x64"])
def test_custom_residual_through_the_drop_in_face(case, monkeypatch):
    layers, loss_fn, N = {"corrected_pe_3x24": ([2, 24, 24, 24, 6], corrected_pe, 400),
                          "corrected_pe_8x64": ([2] + [64] * 8 + [6], corrected_pe, 3001),
                          "burgers_4x20": ([3, 20, 20, 20, 20, 4], burgers, 700),
                          "burgers_8x64": ([3] + [64] * 8 + [4], burgers, 5000)}[case]
    seen = []
    orig = Engine.jet_backward

    def spy(self, params, X, gY, gdY, grad, engine=None):
        seen.append((self.desc.engine, engine))
        return orig(self, params, X, gY, gdY, grad, engine)

    monkeypatch.setattr(Engine, "jet_backward", spy)
    model = dropin_model(layers, seed=3)
    Xh = torch.rand(N, layers[0], generator=torch.Generator().manual_seed(5)) * 2 - 1
    cols = [Xh[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(layers[0])]
    pred = model(torch.cat(cols, -1))
    loss = loss_fn(*cols, *[pred[:, i:i + 1] for i in range(layers[-1])])
    model.zero_grad()
    loss.backward()
    got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
    lo, go = fp64_reference(model, Xh, loss_fn)
    lo = lo.detach()
    rel = rel_l2(got, go)
    print(f"{case}: loss {loss.item():.6e} (fp64 {float(lo):.6e}) grad rel_l2 {rel:.2e}; jet_backward calls {seen}")
    assert abs(loss.item() - float(lo)) / abs(float(lo)) < 5e-6
    assert rel < TOL
    # the reverse sweeps ran on the descriptor's own engine, AUTO, with no override: the MFMA path for these shapes
    assert 1 <= len(seen) <= 2 and all(s == (ENGINE_AUTO, None) for s in seen), seen


def test_dropout_in_training_mode_falls_back_to_the_generic_engine(monkeypatch):
    from pinn_depthestimation_amd.dnn import DNN
    seen = []
    orig = Engine.jet_backward

    def spy(self, params, X, gY, gdY, grad, engine=None):
        seen.append((self, self.dropout_seed, engine, params.clone(), X.clone(), None if gY is None else gY.clone(),
                     None if gdY is None else gdY.clone()))
        return orig(self, params, X, gY, gdY, grad, engine)

    monkeypatch.setattr(Engine, "jet_backward", spy)
    torch.manual_seed(7)
    model = DNN([3, 48, 48, 48, 4], 0.2, "xavier").to("cuda")
    model.train()
    Xh = torch.rand(500, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1
    cols = [Xh[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(3)]
    pred = model(torch.cat(cols, -1))
    loss = burgers(*cols, *[pred[:, i:i + 1] for i in range(4)])
    model.zero_grad()
    loss.backward()
    got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
    assert torch.isfinite(got).all() and 1 <= len(seen) <= 2
    acc = torch.zeros_like(got)
    for eng, seed, engine, params, X, gY, gdY in seen:
        assert eng.desc.dropout_p > 0 and eng.desc.engine == ENGINE_AUTO and engine is None
        eng.dropout_seed = seed
        orig(eng, params, X, gY, gdY, acc, ENGINE_GENERIC)
    assert torch.equal(got, acc)


def test_full_size_fused_against_generic_and_run_to_run():
    desc = NetDesc(3, 4, 8, 64, (0, 1, 2))
    N = (1 << 20) + 5
    g = torch.Generator().manual_seed(21)
    params = O.flatten(O.init_params(desc.layers, "xavier", g)).cuda()
    X = (torch.rand(N, 3, generator=g) * 2 - 1).cuda()
    gY = (torch.randn(N, 4, generator=g) / N).cuda()
    gdY = (torch.randn(3, N, 4, generator=g) / N).cuda()

    def go(engine):
        grad = torch.zeros(desc.n_params, device="cuda")
        Engine(desc.with_(engine=engine)).jet_backward(params, X, gY, gdY, grad)
        torch.cuda.synchronize()
        return grad

    fused, generic = go(ENGINE_FUSED), go(ENGINE_GENERIC)
    rel = float((fused - generic).norm() / generic.norm())
    again = go(ENGINE_FUSED)
    rr = float((again - fused).norm() / fused.norm())
    print(f"N={N}: fused vs generic {rel:.2e}, run to run {rr:.2e}")
    assert rel < 2e-5
    assert rr < 1e-6

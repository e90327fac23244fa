"""The corrected radiation-stress residual (ResidualSpec.corrected, pinn_residual_spec.flags bit 0) on the GPU: loss and
gradient of every engine that serves it against the Python formula of physics.physics_equation(corrected=True) evaluated
with torch autograd in float64 over oracle.mlp_forward on the CPU; both loss terms in one pass; per-point fields; the
folded Adam iteration; the trainer; the drop-in face; the refusals.

Bars (tests/test_engine_gpu.py's): loss max(2e-6, 4 x noise), flat gradient rel_l2 < max(2e-5, 4 x noise), noise = the fp32
run of the same torch formula against its fp64 run.  The networks are conditioned (pe_corrected_util.conditioned_params) so
that the stress terms carry weight: they move the loss by 5 % at 10 x 10 and the gradient by 2-7 %, far outside every bar —
all comparisons here fail on a library that ignores the flag."""
import functools

import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, physics
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16, PinnError)
from tests.pe_corrected_util import ROLES, conditioned_params, net_fields, net_loss_grad, pec_fields, pec_loss, points

pytestmark = pytest.mark.gpu

OUT8 = ("aux0", "k", "h", "U", "aux1", "V", "eta_mean", "Hrms")
NETS = {
    # name: layers, N, outputs, input names, grad_cols, what it covers
    "10x10": ([2] + [10] * 10 + [6], 777, ROLES, ("x", "y"), (0, 1)),              # width 16
    "2x16": ([2, 16, 16, 6], 333, ROLES, ("x", "y"), (0, 1)),                      # four k-steps
    "3x24": ([2, 24, 24, 24, 6], 400, ROLES, ("x", "y"), (0, 1)),                  # width 32
    "3x32": ([2, 32, 32, 32, 6], 333, ROLES, ("x", "y"), (0, 1)),                  # eight k-steps
    "8x64": ([2] + [64] * 8 + [6], 777, ROLES, ("x", "y"), (0, 1)),                # width 64
    "40x20": ([2] + [20] * 40 + [6], 333, ROLES, ("x", "y"), (0, 1)),              # gradient copy in global memory / atomic sink
    "1x10_17": ([2, 10, 6], 17, ROLES, ("x", "y"), (0, 1)),                        # single hidden layer, ragged tile
    "1x10_16": ([2, 10, 6], 16, ROLES, ("x", "y"), (0, 1)),
    "1x10_1": ([2, 10, 6], 1, ROLES, ("x", "y"), (0, 1)),
    "3x12_perm": ([3, 12, 12, 12, 8], 500, OUT8, ("y", "c", "x"), (0, 2)),         # roles out of column order, directions permuted
}
NARROW = [n for n, v in NETS.items() if v[0][1] <= 32]


def _rel_l2(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def case(name, N=None, init_type="xavier", layers=None, inn=None, gc=None):
    """Network, points and the fp64 / fp32 runs of the formula, computed once and shared (nothing below writes to them)."""
    L, n0, outn, inn0, gc0 = NETS[name] if name in NETS else (list(layers), N, ROLES, inn, gc)
    N = N or n0
    params = conditioned_params(L, outn, seed=3, init_type=init_type)
    X = points(N, L[0], seed=5)
    desc = NetDesc.from_layers(L, gc0, ACT_LEAKY_RELU if init_type == "kaiming" else 0)
    spec = ResidualSpec.from_names("physics_equation", inn0, desc.grad_cols, outn, corrected=True)
    kw = dict(xcol=list(inn0).index("x"), ycol=list(inn0).index("y"), outputs=outn, init_type=init_type)
    l64, g64, nl, ng = reference(params, X, kw)
    return desc, spec, O.flatten(params), X, l64, g64, nl, ng, kw


def reference(params, X, kw):
    """fp64 loss and gradient of the formula, and the fp32 run's distance to them (the noise of the bars)."""
    l64, g64 = net_loss_grad(params, X, torch.float64, **kw)
    l32, g32 = net_loss_grad(params, X, torch.float32, **kw)
    return l64, g64, abs(l32 - l64) / abs(l64), float((g32 - g64).norm() / g64.norm())


def check(tag, loss, grad, l64, g64, nl, ng):
    el, eg = abs(loss - l64) / abs(l64), _rel_l2(grad, g64)
    print(f"PEC {tag}: loss {loss:.6e} fp64 {l64:.6e} rel {el:.2e} (noise {nl:.1e}); gradient rel_l2 {eg:.2e} (noise {ng:.1e})")
    assert el < max(2e-6, 4 * nl), (tag, el, nl)
    assert eg < max(2e-5, 4 * ng), (tag, eg, ng)


def run_loss_grad(eng, spec, flat, X, engine=None, base=None):
    N = X.shape[0]
    grad = torch.zeros(flat.numel(), device="cuda") if base is None else base.clone()
    scale = torch.full((3,), 1.0 / N, device="cuda")
    sums = eng.residual_loss_grad(spec, scale, flat, X, grad, engine=engine)
    return sums, float(sums.double().sum()) / N, grad


LOSS_CASES = [(n, e) for n in NETS for e in (ENGINE_GENERIC, ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH)
              if e != ENGINE_FUSED_BATCH or n in NARROW]          # (the batch kernel serves widths up to 32)


@pytest.mark.parametrize("name,engine", LOSS_CASES, ids=[f"{n}-{ {1: 'generic', 4: 'tile', 6: 'batch'}[e]}" for n, e in LOSS_CASES])
def test_loss_and_gradient_against_fp64(name, engine):
    desc, spec, flat, X, l64, g64, nl, ng, _ = case(name)
    eng = Engine(desc.with_(engine=engine))
    fl, Xd = flat.cuda(), X.cuda()
    base = (torch.randn(flat.numel(), generator=torch.Generator().manual_seed(9)) * 0.01).cuda()
    sums, loss, grad = run_loss_grad(eng, spec, fl, Xd, base=base)          # the gradient is ADDED to what grad held
    check(f"{name}/{engine}", loss, grad - base, l64, g64, nl, ng)
    # the flag matters: the plain residual on the same network is far away
    plain = ResidualSpec(spec.name, spec.out_col, spec.dir_of)
    _, lp, gp = run_loss_grad(eng, plain, fl, Xd)
    assert _rel_l2(gp, g64) > 1e-3
    # residual_loss alone gives the gradient call's sums
    s0 = eng.residual_loss(spec, fl, Xd)
    assert torch.allclose(s0, sums, rtol=1e-6), (s0, sums)
    # a dirty workspace changes nothing
    ws = eng.workspace(X.shape[0])
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(1e30)
    sums2, loss2, grad2 = run_loss_grad(eng, spec, fl, Xd)
    assert torch.allclose(sums2, sums, rtol=1e-6)
    check(f"{name}/{engine}/dirty-ws", loss2, grad2, l64, g64, nl, ng)
    # Hrms and k receive a gradient (the bug-compatible residual gives them exactly none)
    W_last = grad2[desc.n_params - desc.d_out * (desc.width + 1): desc.n_params - desc.d_out].view(desc.d_out, desc.width)
    Wp_last = gp[desc.n_params - desc.d_out * (desc.width + 1): desc.n_params - desc.d_out].view(desc.d_out, desc.width)
    for role in ("Hrms", "k"):
        row = spec.out_col[ROLES.index(role)]
        assert float(W_last[row].abs().max()) > 0 and float(Wp_last[row].abs().max()) == 0


@pytest.mark.parametrize("name,per_wave", [("10x10", 8), ("4x20", 4)])
def test_full_batch_instances_under_auto(name, per_wave):
    """The smallest N at which every wave of the chip gets a full batch (batch_T_for: tiles >= CUs x 4 waves x occupancy x
    T; occupancy x T = 8 at width 16, 4 at width 32), plus 5: 131 077 / 65 541 points on an MI355X."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * cus * 4 * per_wave + 5
    layers = (2,) + ((10,) * 10 if name == "10x10" else (20,) * 4) + (6,)
    desc, spec, flat, X, l64, g64, nl, ng, _ = case("full_" + name, N, "xavier", layers, ("x", "y"), (0, 1))
    _, loss, grad = run_loss_grad(Engine(desc), spec, flat.cuda(), X.cuda())
    check(f"full batch {name} N={N}", loss, grad, l64, g64, nl, ng)


# ---- both loss terms ---------------------------------------------------------------------------------------------------
def _fid_reference(params, X, T, cols, kw):
    p = [q.double().requires_grad_(True) for q in params]
    l = O.fidelity_loss(p, X.double(), T.double(), cols, [1.0] * len(cols), kw["init_type"])
    return float(l), O.flat_grad(l, p)


@pytest.mark.parametrize("engine", [ENGINE_AUTO, ENGINE_GENERIC, ENGINE_FUSED_BATCH], ids=["auto", "generic", "batch"])
def test_residual_and_fidelity_on_one_point_set(engine):
    desc, spec, flat, X, l64, g64, nl, ng, kw = case("10x10")
    N, cols = X.shape[0], [0, 3]
    T = torch.rand(N, 2, generator=torch.Generator().manual_seed(4))
    lf, gf = _fid_reference(O.unflatten(flat, desc.layers), X, T, cols, kw)
    eng = Engine(desc.with_(engine=engine))
    grad = torch.zeros(flat.numel(), device="cuda")
    sc, cs = torch.full((3,), 1.0 / N, device="cuda"), torch.full((2,), 1.0 / N, device="cuda")
    ts, cc = eng.residual_mse_loss_grad(spec, sc, T.cuda(), cols, cs, flat.cuda(), X.cuda(), grad)
    loss = (float(ts.double().sum()) + float(cc.double().sum())) / N
    check(f"one set/{engine}", loss, grad, l64 + lf, g64 + gf, nl, ng)


@pytest.mark.parametrize("engine", [ENGINE_AUTO, ENGINE_FUSED_TILE, ENGINE_GENERIC], ids=["auto", "tile", "generic"])
@pytest.mark.parametrize("name", ["10x10", "3x24", "8x64"])
def test_split_pass_equals_the_two_calls_and_fp64(name, engine):
    desc, spec, flat, _, _, _, _, _, kw = case(name)
    nr, nf, cols = 243, 12, [1, 4]
    X = points(nr + nf, 2, seed=6)
    T = torch.rand(nf, 2, generator=torch.Generator().manual_seed(4))
    params = O.unflatten(flat, desc.layers)
    l64, g64, nl, ng = reference(params, X[:nr], kw)
    lf, gf = _fid_reference(params, X[nr:], T, cols, kw)
    eng = Engine(desc.with_(engine=engine))
    fl, Xd, Td = flat.cuda(), X.cuda(), T.cuda()
    sc, cs = torch.full((3,), 1.0 / nr, device="cuda"), torch.full((2,), 1.0 / nf, device="cuda")
    g2 = torch.zeros(flat.numel(), device="cuda")
    ts, cc = eng.residual_mse_split_loss_grad(spec, sc, Td, cols, cs, fl, Xd, nr, g2)
    g1 = torch.zeros(flat.numel(), device="cuda")
    s_res = eng.residual_loss_grad(spec, sc, fl, Xd[:nr].contiguous(), g1)
    s_mse = eng.mse_loss_grad(fl, Xd[nr:].contiguous(), Td, cols, cs, g1)
    assert torch.allclose(ts, s_res, rtol=2e-6) and torch.allclose(cc, s_mse, rtol=2e-6), (ts, s_res, cc, s_mse)
    rel = _rel_l2(g2, g1.double().cpu())
    print(f"PEC split {name}/{engine}: one pass vs two calls rel_l2 {rel:.2e}")
    assert rel < 3e-6
    check(f"split {name}/{engine}", float(ts.double().sum()) / nr + float(cc.double().sum()) / nf, g2, l64 + lf, g64 + gf, nl, ng)


# ---- fields ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [ENGINE_AUTO, ENGINE_GENERIC], ids=["tile", "staged"])
@pytest.mark.parametrize("name", ["10x10", "3x24", "8x64", "1x10_17", "3x12_perm"])
def test_fields_against_fp64_and_the_loss_sums(name, engine):
    desc, spec, flat, X, _, _, _, _, kw = case(name)
    params = O.unflatten(flat, desc.layers)
    f64 = net_fields(params, X, dtype=torch.float64, **kw)[0].detach()
    f32 = net_fields(params, X, dtype=torch.float32, **kw)[0].detach().double()
    eng = Engine(desc.with_(engine=engine))
    got = eng.residual_fields(spec, flat.cuda(), X.cuda())
    assert got.shape == (3, X.shape[0]) and got.dtype == torch.float32
    err = (got.cpu().double() - f64).abs().amax(1)
    noise = (f32 - f64).abs().amax(1)
    floor = 2.0 ** -23 * f64.abs().amax(1)
    print(f"PEC fields {name}/{engine}: err {[f'{e:.2e}' for e in err.tolist()]} noise {[f'{e:.2e}' for e in noise.tolist()]}")
    assert bool((err <= 4 * torch.maximum(noise, floor)).all()), (err.tolist(), noise.tolist(), floor.tolist())     # test_fields_gpu.py's bar
    sums = eng.residual_loss(spec, flat.cuda(), X.cuda()).cpu().double()
    assert torch.allclose(got.cpu().double().square().sum(1), sums, rtol=1e-5)
    plain = eng.residual_fields(ResidualSpec(spec.name, spec.out_col, spec.dir_of), flat.cuda(), X.cuda())
    assert float((plain[1:] - got[1:]).abs().max()) > 1e-3 and torch.allclose(plain[0], got[0], rtol=1e-6, atol=1e-7)     # fc has no stress term


# ---- folded Adam ---------------------------------------------------------------------------------------------------------
def test_folded_iteration_alternating_plain_and_corrected_on_one_engine():
    """At width 64 the plain residual-only pass of the tile kernel reads its weights packed k-step-major, the corrected one
    in natural order: the packed copy one call leaves behind must not be reused by the other (Engine's packed-copy token
    carries the spec).  5000 points: above the cooperative kernel's range, which packs in natural order for both."""
    desc, spec, flat, *_ = case("8x64")
    plain = ResidualSpec(spec.name, spec.out_col, spec.dir_of)
    N, P = 5000, flat.numel()
    Xd = points(N, 2, seed=12).cuda()
    sc = torch.full((3,), 1.0 / N, device="cuda")
    shared = Engine(desc)
    th, m, v = flat.cuda().clone(), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    for i, sp in enumerate((plain, spec, plain, spec)):
        th_b, m_b, v_b = th.clone(), m.clone(), v.clone()
        g_a, g_b, ts_a, ts_b = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda"), torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
        assert shared.loss_grad_adam_step(sp, sc, th, Xd, N, g_a, m, v, i + 1, 1e-3, term_sums=ts_a)
        assert Engine(desc).loss_grad_adam_step(sp, sc, th_b, Xd, N, g_b, m_b, v_b, i + 1, 1e-3, term_sums=ts_b)
        rel = _rel_l2(g_a, g_b.double().cpu())
        print(f"PEC alternating call {i} ({'corrected' if sp.corrected else 'plain'}): gradient rel_l2 shared vs fresh engine {rel:.2e}")
        assert torch.allclose(ts_a, ts_b, rtol=1e-5), (i, ts_a, ts_b)
        assert rel < 5e-6, i
        assert torch.allclose(th, th_b, rtol=2e-4, atol=1e-7), i


def test_three_folded_iterations_equal_loss_call_plus_adam_step():
    desc, spec, flat, X, *_ = case("8x64")
    Xd, N, P = X.cuda(), X.shape[0], flat.numel()
    sc = torch.full((3,), 1.0 / N, device="cuda")
    out = []
    for folded in (False, True):
        eng = Engine(desc)
        th, m, v, g, ts = flat.cuda().clone(), *(torch.zeros(P, device="cuda") for _ in range(3)), torch.zeros(3, device="cuda")
        for it in (1, 2, 3):
            if folded:
                assert eng.loss_grad_adam_step(spec, sc, th, Xd, N, g, m, v, it, 1e-3, term_sums=ts)
            else:
                g.zero_(); eng.residual_loss_grad(spec, sc, th, Xd, g, sums=ts); eng.adam_step(th, g, m, v, it, 1e-3)
        out.append(th.clone())
    rel = _rel_l2(out[1], out[0].double().cpu())
    print(f"PEC folded vs classic parameters after 3 iterations: rel_l2 {rel:.2e}")
    assert rel < 1e-6 and float((out[1] - flat.cuda()).abs().max()) > 0


# ---- trainer -------------------------------------------------------------------------------------------------------------
def _cfg(L, W, steps, **loss):
    return {"layers": {"input_features": 2, "hidden_layers": L, "hidden_width": W, "output_features": 6},
            "adam_optimizer": {"max_it": steps, "learning_rate": 1e-3, "scheduler_step_size": 10000, "scheduler_gamma": 0.8},
            "lbfgs_optimizer": {"max_it": 0}, "loss": dict({"weight_fid_loss": 1, "weight_res_loss": 1}, **loss),
            "data_fidelity": {"inputs": ["x", "y"], "outputs": ["h", "U"]},
            "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"}, "outputs": list(ROLES)}}


def _dnn(layers, params):
    from pinn_depthestimation_amd.dnn import DNN
    model = DNN(layers, 0.0, "xavier").to("cuda")
    with torch.no_grad():
        for p, q in zip(model._ordered_params(), params):
            p.copy_(q)
    return model


@functools.lru_cache(maxsize=None)
def _trajectory(name):
    """30 Adam steps at lr 1e-3 on the formula (O.adam_trajectory): the fp64 losses and the fp32 run's gap to them."""
    desc, spec, flat, _, _, _, _, _, kw = case(name)
    Xr, Xf = points(243, 2, seed=7), points(12, 2, seed=8)
    Tf = torch.rand(12, 2, generator=torch.Generator().manual_seed(4))
    params = O.unflatten(flat, desc.layers)

    def run(dt):
        def loss_fn(p):
            f = net_fields_with(p, Xr.to(dt))
            return O.fidelity_loss(p, Xf.to(dt), Tf.to(dt), [0, 1], [1.0, 1.0]) + (f ** 2).mean(dim=1).sum()
        return np.array(O.adam_trajectory([q.to(dt) for q in params], loss_fn, 30, 1e-3)[0])

    def net_fields_with(p, X):
        cols = O.split_columns(X, (0, 1))
        Y = O.mlp_forward(p, torch.cat(cols, dim=-1))
        return torch.cat(pec_fields(cols[0], cols[1], *[Y[:, r:r + 1] for r in range(6)]), dim=1).t()

    l64, l32 = run(torch.float64), run(torch.float32)
    return params, Xr, Xf, Tf, l64, float(np.max(np.abs(l32 - l64) / np.abs(l64)))


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "classic"])
@pytest.mark.parametrize("name", ["10x10", "8x64"])
def test_trainer_walks_the_fp64_trajectory(name, fold):
    from pinn_depthestimation_amd.trainer import PINN
    desc, *_ = case(name)
    params, Xr, Xf, Tf, l64, gap = _trajectory(name)
    tr = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), _cfg(desc.n_hidden, desc.width, 30), dnn=_dnn(desc.layers, params), log_every=1,
              checkpoint_every=0, fold_adam=fold, corrected=True)
    assert tr.spec.corrected and tr.evaluator.spec.corrected
    tr.train_adam(30)
    got = np.array([r[3] for r in tr.history])
    rel = np.abs(got - l64) / np.abs(l64)
    print(f"PEC trainer {name} fold={fold}: max rel loss error {rel.max():.2e} (fp32 gap {gap:.2e}), folded iterations {tr._folded_iters}")
    assert len(got) == 30 and float(rel.max()) < max(1e-5, 4 * gap)
    assert (tr._folded_iters > 0) == fold
    assert got[-1] < got[0]


def test_trainer_reads_the_config_key_and_rad_scores_with_the_corrected_fields(monkeypatch):
    from pinn_depthestimation_amd.trainer import PINN
    desc, spec, flat, X, *_ = case("10x10")
    seen = []
    orig = Engine.residual_fields

    def spy(self, sp, params, Xs, engine=None):
        out = orig(self, sp, params, Xs, engine)
        seen.append((sp.corrected, out.clone(), Xs.clone(), params.clone()))
        return out

    monkeypatch.setattr(Engine, "residual_fields", spy)
    tr = PINN(None, None, X.numpy(), dict(_cfg(10, 10, 4, corrected_radiation_stress=True), data_fidelity={"inputs": ["x", "y"], "outputs": []}),
              dnn=_dnn(desc.layers, O.unflatten(flat, desc.layers)), checkpoint_every=0, residual_batch=128, resample="rad", rad_every=2)
    assert tr.corrected
    for _ in range(4):
        tr.adam_step()
    assert len(seen) == 2 and all(s[0] for s in seen)
    assert tr._rad_score is not None and bool(torch.isfinite(tr._rad_score).all()) and bool(torch.isfinite(tr.last[2]))
    # the first scoring ran at the initial parameters: its fields are the corrected ones of the fp64 formula
    f64 = net_fields(O.unflatten(flat, desc.layers), X, dtype=torch.float64)[0].detach()
    assert float((seen[0][1].cpu().double() - f64).abs().max()) < 1e-4 * float(f64.abs().max())


# ---- drop-in face --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["10x10", "8x64"])
def test_drop_in_physics_equation_corrected(name, monkeypatch):
    desc, spec, flat, X, l64, g64, nl, ng, _ = case(name)
    calls = []
    orig = Engine.jet_backward
    monkeypatch.setattr(Engine, "jet_backward", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    out = {}
    for tag, fn in (("hard-wired", physics.physics_equation_corrected),
                    ("formula", lambda *a: physics.physics_equation(*a, corrected=True))):
        model = _dnn(desc.layers, O.unflatten(flat, desc.layers))
        cols = [X[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(2)]
        pred = model(torch.cat(cols, -1))
        n0 = len(calls)
        loss = fn(*cols, *[pred[:, i:i + 1] for i in range(6)])
        model.zero_grad()
        loss.backward()
        grad = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        out[tag] = (loss.item(), grad, len(calls) - n0)
    assert out["hard-wired"][2] == 0 and out["formula"][2] >= 1        # no jet_backward call on the hard-wired path
    check(f"drop-in hard-wired {name}", out["hard-wired"][0], out["hard-wired"][1], l64, g64, nl, ng)
    # ... and it is the loss and p.grad of physics_equation(corrected=True) (that path's own bars, test_jet_backward_mfma_gpu.py)
    assert abs(out["formula"][0] - l64) / abs(l64) < 5e-6 and _rel_l2(out["formula"][1], g64) < 5e-5
    assert abs(out["hard-wired"][0] - out["formula"][0]) <= 5e-6 * abs(l64)
    assert _rel_l2(out["hard-wired"][1], out["formula"][1].double().cpu()) < 5e-5


def test_drop_in_falls_back_to_the_formula():
    # plain CPU float64 tensors
    x = torch.rand(20, 1, dtype=torch.float64).requires_grad_(True)
    y = torch.rand(20, 1, dtype=torch.float64).requires_grad_(True)
    outs = [c + 0.1 * x * (i + 1) - 0.2 * y for i, c in enumerate((2.0, 0.1, -0.2, 0.2, 0.5, 1.0))]
    assert float(physics.physics_equation_corrected(x, y, *outs).detach()) == float(pec_loss(x, y, *outs).detach())
    # a LeakyReLU network: the fused engine has no such instance, the formula runs (forward jet + autograd + jet_backward)
    from pinn_depthestimation_amd.dnn import DNN
    torch.manual_seed(2)
    model = DNN([2, 20, 20, 6], 0.0, "kaiming").to("cuda")
    last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.weight.mul_(0.25); last.bias.copy_(torch.tensor([2.0, 0.0, 0.0, 0.2, 0.5, 1.0]))
    cols = [points(100, 2)[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(2)]
    pred = model(torch.cat(cols, -1))
    a = physics.physics_equation_corrected(*cols, *[pred[:, i:i + 1] for i in range(6)])
    b = physics.physics_equation(*cols, *[pred[:, i:i + 1] for i in range(6)], corrected=True)
    assert a.item() == pytest.approx(b.item(), rel=1e-6)


# ---- refusals and the generic engine's reach ---------------------------------------------------------------------------
@pytest.mark.parametrize("case_name,desc", [
    ("width 100, AUTO", NetDesc(2, 6, 3, 100, (0, 1))),
    ("width 100, WIDE", NetDesc(2, 6, 3, 100, (0, 1), engine=ENGINE_WIDE)),
    ("bf16", NetDesc(2, 6, 3, 128, (0, 1), precision=PREC_BF16)),
    ("LeakyReLU, FUSED", NetDesc(2, 6, 3, 20, (0, 1), activation=ACT_LEAKY_RELU, engine=ENGINE_FUSED)),
    ("k = 3, FUSED", NetDesc(3, 6, 3, 20, (0, 1, 2), engine=ENGINE_FUSED)),
])
def test_refusals_through_the_engine(case_name, desc):
    inn = ("x", "y", "t") if desc.k == 3 else ("x", "y")
    spec = ResidualSpec.from_names("physics_equation", inn, desc.grad_cols, ROLES, corrected=True)
    eng = Engine(desc)
    flat = torch.zeros(desc.n_params, device="cuda")
    X = points(64, desc.d_in).cuda()
    grad, sc = torch.zeros_like(flat), torch.ones(3, device="cuda")
    with pytest.raises(PinnError, match="corrected"):
        eng.residual_loss_grad(spec, sc, flat, X, grad)
    with pytest.raises(PinnError, match="corrected"):
        eng.residual_loss(spec, flat, X)
    m, v, ts = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(3, device="cuda")
    assert eng.loss_grad_adam_step(spec, sc, flat, X, 64, grad, m, v, 1, 1e-3, term_sums=ts) is False
    assert float(grad.abs().max()) == 0.0 and float(flat.abs().max()) == 0.0
    if "FUSED" in case_name:
        with pytest.raises(PinnError, match="corrected"):
            eng.residual_fields(spec, flat, X)


@pytest.mark.parametrize("which", ["leaky", "k3", "dropout_auto"])
def test_generic_engine_serves_what_the_fused_engine_refuses(which):
    if which == "leaky":
        desc, spec, flat, X, l64, g64, nl, ng, _ = case("leaky_3x20", 333, "kaiming", (2, 20, 20, 20, 6), ("x", "y"), (0, 1))
    elif which == "k3":
        desc, spec, flat, X, l64, g64, nl, ng, _ = case("k3_3x20", 333, "xavier", (3, 20, 20, 20, 6), ("x", "y", "t"), (0, 1, 2))
    else:
        desc, spec, flat, X, l64, g64, nl, ng, _ = case("8x64")
    if which == "dropout_auto":
        # AUTO with dropout: the generic engine (the fused dropout instances do not carry the corrected residual); FUSED refused
        d = desc.with_(dropout_p=0.25)
        eng = Engine(d)
        eng.dropout_seed = 7
        sums, loss, grad = run_loss_grad(eng, spec, flat.cuda(), X.cuda())
        ref = Engine(d.with_(engine=ENGINE_GENERIC))
        ref.dropout_seed = 7
        sums_r, loss_r, grad_r = run_loss_grad(ref, spec, flat.cuda(), X.cuda())
        assert torch.equal(sums, sums_r) and torch.equal(grad, grad_r) and np.isfinite(loss)
        with pytest.raises(PinnError, match="corrected"):
            run_loss_grad(Engine(d.with_(engine=ENGINE_FUSED)), spec, flat.cuda(), X.cuda())
        return
    _, loss, grad = run_loss_grad(Engine(desc.with_(engine=ENGINE_GENERIC)), spec, flat.cuda(), X.cuda())
    check(f"generic {which}", loss, grad, l64, g64, nl, ng)


def test_fused_coop_runs_the_tile_kernel():
    desc, spec, flat, X, l64, g64, nl, ng, _ = case("8x64")
    _, loss, grad = run_loss_grad(Engine(desc.with_(engine=ENGINE_FUSED_COOP)), spec, flat.cuda(), X.cuda()[:243].contiguous())
    l, g = net_loss_grad(O.unflatten(flat, desc.layers), X[:243])
    check("FUSED_COOP 8x64 N=243", loss, grad, l, g, nl, ng)

"""Per-point weights on the PDE residual on the GPU: pinn_residual_weighted_loss_grad (the tile kernel's weighted instances,
the generic engine, AUTO) against torch autograd over the formulas evaluated with the weights, in float64 and float32
(tests/weighted_util.py); forward-only bit equality, w == 1 against the unweighted entries, zero weights, the buffer
contract, reproducibility, the engine rules, and the trainer (self-adaptive weights, a fixed mask, RAD importance weights).

Bounds (tests/weighted_util.py): term sums by sweep2_util.sum_ratio <= 1; parameter gradient per block by max(2e-5, 4 gap)
(assert_blocks_close); fields by sweep2_util.field_ratios <= FIELD_BOUND."""
import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ACT_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16, PinnError)
from tests import abi_contract_util as A
from tests import weighted_util as U

pytestmark = pytest.mark.gpu

ENGINES = {"tile": ENGINE_FUSED_TILE, "generic": ENGINE_GENERIC, "auto": ENGINE_AUTO}


def setup(shape):
    c = U.shape_case(shape)
    desc = NetDesc.from_layers(c.layers, tuple(range(c.d_in)), ACT_TANH if c.init == "xavier" else ACT_LEAKY_RELU)
    spec = ResidualSpec.from_names(c.res, c.inn, desc.grad_cols, c.outn)
    assert (spec.threshold, spec.anchor) == (U.S.THRESHOLD, U.S.ANCHOR)
    return c, desc, spec, Engine(desc, "cuda")


def names_of(shape):
    return ("generic", "auto") if shape in U.GENERIC_ONLY else ("tile", "generic", "auto")


def run(eng, spec, shape, N, w, engine, grad=True, fields=True, X=None):
    params, X0 = U.inputs(shape, N)
    flat, Xd = O.flatten(params).cuda(), (X0 if X is None else X).cuda()
    scale = torch.tensor(U.scale_of(shape, N), dtype=torch.float32, device="cuda")
    g = torch.zeros_like(flat) if grad else None
    out = eng.residual_weighted_loss_grad(spec, w.cuda(), scale if grad else None, flat, Xd, g, fields=True if fields else None,
                                          engine=engine)
    torch.cuda.synchronize()
    sums, F = out if fields else (out, None)
    return sums, g, F


# ---- sums, gradient and fields against the fp64 formula; forward only ----------------------------------------------------------
@pytest.mark.parametrize("shape,N", U.cases())
def test_sums_gradient_and_fields(shape, N):
    c, desc, spec, eng = setup(shape)
    for wr in U.w_rows_of(shape):
        r64, r32 = U.reference(shape, N, wr)
        w = U.weights(shape, N, wr)
        for name in names_of(shape):
            what = f"{shape} N={N} w_rows={wr} {name}"
            sums, g, F = run(eng, spec, shape, N, w, ENGINES[name])
            rs, rf = U.sums_ratio(sums, r64, r32), U.field_ratio(F, r64)
            print(f"{what}: sums {rs:.3f}, fields {rf:.3f}")
            rg = U.grad_ratio(g, r64, r32, c.layers, what)
            print(f"{what}: gradient {rg:.3f}")
            assert rs <= 1.0, (what, sums.tolist(), r64.sums.tolist(), rs)
            assert rf <= U.FIELD_BOUND, (what, rf)
            if c.res == "continuity_only":
                assert float(sums[2]) == float(r64.sums[2]), (what, "the count is not weighted", float(sums[2]), float(r64.sums[2]))
            # forward only, with and without the fields: the gradient call's sums bit for bit, the same fields
            fwd, g0, F0 = run(eng, spec, shape, N, w, ENGINES[name], grad=False)
            fwd1, _, F1 = run(eng, spec, shape, N, w, ENGINES[name], grad=False, fields=False)
            assert g0 is None and F1 is None
            assert torch.equal(fwd, sums) and torch.equal(fwd1, sums), (what, fwd.tolist(), fwd1.tolist(), sums.tolist())
            assert U.field_ratio(F0, r64) <= U.FIELD_BOUND, what
            # the gradient call without the fields: the same sums, a gradient within the bound
            s2, g2, _ = run(eng, spec, shape, N, w, ENGINES[name], fields=False)
            assert torch.equal(s2, sums), (what, s2.tolist(), sums.tolist())
            U.grad_ratio(g2, r64, r32, c.layers, what + " fields=None")


# ---- w == 1: the unweighted entries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.TILE_SHAPES + U.GENERIC_ONLY)
def test_unit_weights_agree_with_the_unweighted_entries(shape):
    c, desc, spec, eng = setup(shape)
    for N in (17, 243, 4097):
        params, X = U.inputs(shape, N)
        flat, Xd = O.flatten(params).cuda(), X.cuda()
        scale = torch.tensor(U.scale_of(shape, N), dtype=torch.float32, device="cuda")
        for wr in U.w_rows_of(shape):
            r64, r32 = U.reference(shape, N, wr, True)
            for name in [n for n in names_of(shape) if n != "auto"]:
                what = f"{shape} N={N} w_rows={wr} {name} w=1"
                sums, g, F = run(eng, spec, shape, N, torch.ones(wr, N), ENGINES[name])
                g0 = torch.zeros_like(flat)
                s0 = eng.residual_loss_grad(spec, scale, flat, Xd, g0, engine=ENGINES[name])
                F0 = eng.residual_fields(spec, flat, Xd, engine=ENGINES[name])
                torch.cuda.synchronize()
                for got in (sums, s0):
                    assert U.sums_ratio(got, r64, r32) <= 1.0, (what, got.tolist(), r64.sums.tolist())
                U.grad_ratio(g, r64, r32, c.layers, what)
                U.grad_ratio(g0, r64, r32, c.layers, what + " residual_loss_grad")
                assert U.field_ratio(F, r64) <= U.FIELD_BOUND and U.field_ratio(F0, r64) <= U.FIELD_BOUND, what


# ---- a zero weight removes the point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,N", [(s, n) for s in U.TILE_SHAPES + U.GENERIC_ONLY for n in (17, 243, 4097)])
def test_a_zero_weight_removes_the_point(shape, N):
    c, desc, spec, eng = setup(shape)
    w = U.weights(shape, N, 1)
    params, X = U.inputs(shape, N)
    zero = (w[0] == 0)
    assert 0 < int(zero.sum()) < N
    g = torch.Generator().manual_seed(N)
    X2 = X.clone()
    X2[zero] = U._draw_x(c, int(zero.sum()), g)                      # other in-range points where the weight is zero
    r64, r32 = U.reference(shape, N, 1)
    for name in [n for n in names_of(shape) if n != "auto"]:
        what = f"{shape} N={N} {name}"
        s1, g1, F1 = run(eng, spec, shape, N, w, ENGINES[name])
        s2, g2, F2 = run(eng, spec, shape, N, w, ENGINES[name], X=X2)
        nw = U.n_w(shape)
        assert torch.equal(s1[:nw], s2[:nw]), (what, s1.tolist(), s2.tolist())
        if name == "generic" and N <= 512:
            assert torch.equal(g1, g2), what
        else:
            U.grad_ratio(g2, r64, r32, c.layers, what + " replaced points")
        keep = (~zero).cuda()
        assert torch.equal(F1[:, keep], F2[:, keep]), what
        assert not torch.equal(F1[:, ~keep], F2[:, ~keep]), what


# ---- buffer contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tile", "generic"])
@pytest.mark.parametrize("shape", ["pe_10x10", "ns_64x64", "co_20x20"])
def test_buffer_contract(shape, name):
    c, desc, spec, eng = setup(shape)
    N, engine, wr = 243, ENGINES[name], U.n_w(shape)
    params, X = U.inputs(shape, N)
    flat, Xd = O.flatten(params).cuda(), X.cuda()
    scale = torch.tensor(U.scale_of(shape, N), dtype=torch.float32, device="cuda")
    w = U.weights(shape, N, wr)
    sums0, g0, F0 = run(eng, spec, shape, N, w, engine)
    wbuf, wchk = A.guarded((wr, N), device="cuda", name="point_w")
    wbuf.copy_(w.cuda())
    wsnap = A.snapshot(wbuf)
    fbuf, fchk = A.guarded((spec.n_fields, N), device="cuda", name="fields")           # poisoned: must be overwritten
    sbuf, schk = A.guarded(spec.n_terms, device="cuda", name="term_sums")
    pre = torch.linspace(-1, 1, flat.numel())
    gbuf, gchk = A.guarded(flat.numel(), device="cuda", name="grad_flat")
    gbuf.copy_(pre.cuda())                                                               # a non-zero start: +=
    ws = A.poison_workspace(eng.residual_weighted_workspace(spec, N, engine))
    eng.residual_weighted_loss_grad(spec, wbuf, scale, flat, Xd, gbuf, sums=sbuf, fields=fbuf, engine=engine)
    torch.cuda.synchronize()
    for chk in (wchk, fchk, schk, gchk):
        chk.assert_bands_intact()
    A.assert_unchanged(wbuf, wsnap, "point_w")
    assert torch.equal(sbuf, sums0) and torch.equal(fbuf, F0)                            # overwritten; nothing of the workspace read
    r64, r32 = U.reference(shape, N, wr)
    assert bool(torch.isfinite(gbuf).all())
    U.grad_ratio(gbuf - pre.cuda(), r64, r32, c.layers, f"{shape} {name} += onto a non-zero start")
    # N = 0 zeroes term_sums and touches nothing else
    g2, s2 = pre.cuda().clone(), torch.full((spec.n_terms,), 1e30, device="cuda")
    f2 = torch.full((spec.n_fields, 0), 1e30, device="cuda")
    eng.residual_weighted_loss_grad(spec, wbuf[:, :0].contiguous(), scale, flat, Xd[:0], g2, sums=s2, fields=f2, engine=engine)
    torch.cuda.synchronize()
    assert s2.tolist() == [0.0] * spec.n_terms and torch.equal(g2, pre.cuda())


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pe_10x10", "ns_64x64", "co_20x20"])
def test_term_sums_and_fields_are_bit_reproducible(shape):
    c, desc, spec, eng = setup(shape)
    w = U.weights(shape, 4097, U.n_w(shape))
    for name in ("tile", "generic"):
        a = run(eng, spec, shape, 4097, w, ENGINES[name])
        b = run(eng, spec, shape, 4097, w, ENGINES[name])
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), (shape, name)


# ---- engine rules on a device, one case per row of the header's table ------------------------------------------------------------
def _refused(eng, spec, N, engine, word, w_rows=1, code=-2):
    flat = torch.zeros(eng.n_params, device="cuda")
    X = torch.zeros(N, eng.desc.d_in, device="cuda")
    with pytest.raises(PinnError) as e:
        eng.residual_weighted_loss_grad(spec, torch.ones(w_rows, N, device="cuda"), None, flat, X, engine=engine)
    assert word in str(e.value) and f"(code {code})" in str(e.value), str(e.value)


def test_engine_rules():
    pe_out = ("h", "U", "V", "eta_mean", "Hrms", "k")
    # k != the residual's directions
    desc = NetDesc.from_layers([3, 10, 10, 6], (0, 1, 2))
    spec = ResidualSpec.from_names("physics_equation", ("x", "y", "t"), desc.grad_cols, pe_out)
    _refused(Engine(desc, "cuda"), spec, 16, ENGINE_AUTO, "directions")
    # corrected stress
    desc = NetDesc.from_layers([2, 10, 10, 6], (0, 1))
    spec_c = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, pe_out, corrected=True)
    _refused(Engine(desc, "cuda"), spec_c, 16, ENGINE_AUTO, "corrected")
    spec = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, pe_out)
    eng = Engine(desc, "cuda")
    # FUSED_COOP, FUSED_BATCH, WIDE: no such instances
    _refused(eng, spec, 16, ENGINE_FUSED_COOP, "tile kernel")
    _refused(eng, spec, 16, ENGINE_FUSED_BATCH, "tile kernel")
    _refused(eng, spec, 16, ENGINE_WIDE, "wide engine")
    # bf16
    dbf = NetDesc.from_layers([2, 128, 128, 6], (0, 1), precision=PREC_BF16)
    _refused(Engine(dbf, "cuda"), spec, 16, ENGINE_AUTO, "bf16")
    # FUSED refuses what the tile instances do not serve, with the reason; AUTO and GENERIC serve it
    for d, word in ((NetDesc.from_layers([2, 100, 100, 6], (0, 1)), "width"),
                    (NetDesc.from_layers([2, 12, 12, 6], (0, 1), ACT_LEAKY_RELU), "LeakyReLU"),
                    (NetDesc.from_layers([2, 12, 12, 6], (0, 1), dropout_p=0.1), "dropout")):
        e = Engine(d, "cuda")
        _refused(e, spec, 16, ENGINE_FUSED, word)
        flat, X = torch.randn(e.n_params, device="cuda") * 0.3, torch.rand(16, 2, device="cuda")
        for engine in (ENGINE_AUTO, ENGINE_GENERIC):
            s = e.residual_weighted_loss_grad(spec, torch.ones(16, device="cuda"), None, flat, X, engine=engine)
            assert bool(torch.isfinite(s).all())
    # w_rows: 1 or n_w
    for wr in (2, 4):
        _refused(eng, spec, 16, ENGINE_AUTO, "w_rows", w_rows=wr, code=-1)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
LAYERS = [2, 10, 10, 6]
OUTN = ("h", "U", "V", "eta_mean", "Hrms", "k")
LR, LR_W, STEP, GAMMA, ITERS = 1e-3, 1e-2, 7, 0.8, 20
N_RES, N_FID = 243, 12


def _cfg(lbfgs_it=0, **loss):
    return {
        "layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0, "init_type": "xavier"},
        "adam_optimizer": {"max_it": ITERS, "learning_rate": LR, "weight_learning_rate": LR_W, "scheduler_step_size": STEP, "scheduler_gamma": GAMMA},
        "lbfgs_optimizer": {"max_it": lbfgs_it, "learning_rate": 1, "max_evaluation": 12, "history_size": 10,
                            "tolerance_grad": 1e-9, "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1, **{f"weight_{k}_loss": 1 for k in OUTN}, **loss},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": list(OUTN), "training_points": N_FID},
        "data_residual": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}}, "outputs": list(OUTN)},
    }


def _trainer_data():
    from tests.residual2_util import conditioned_params
    g = torch.Generator().manual_seed(78)
    params = conditioned_params(LAYERS, "physics_equation", OUTN, seed=12)
    Xr, Xf = torch.rand(N_RES, 2, generator=g) * 2 - 1, torch.rand(N_FID, 2, generator=g) * 2 - 1
    Tf = torch.rand(N_FID, 6, generator=g)
    return params, Xf, Tf, Xr


def _model(params):
    from pinn_depthestimation_amd.dnn import DNN
    m = DNN(LAYERS, 0.0, "xavier")
    with torch.no_grad():
        for i, lin in enumerate(m._linears()):
            lin.weight.copy_(params[2 * i]); lin.bias.copy_(params[2 * i + 1])
    return m


def _sa_loop(params, Xf, Tf, Xr, mask, dtype):
    """The self-adaptive algorithm in torch: torch.optim.Adam on the network (descent) and on lambda (ascent: its gradient
    negated), one StepLR for both; (total loss per iteration, final lambda (3, N), f^2 of the last pass (3, N))."""
    from tests.coef_util import formula
    p = [q.detach().clone().to(dtype).requires_grad_(True) for q in params]
    lam = torch.ones(3, Xr.shape[0], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([{"params": p, "lr": LR}, {"params": [lam], "lr": LR_W}])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=STEP, gamma=GAMMA)
    Xf_, Tf_ = Xf.to(dtype), Tf.to(dtype)
    losses, f2 = [], None
    for _ in range(ITERS):
        opt.zero_grad()
        fid = ((Tf_ - O.mlp_forward(p, Xf_)) ** 2).mean(0).sum()
        cols = [Xr[:, i:i + 1].to(dtype).requires_grad_(True) for i in range(2)]
        Y = O.mlp_forward(p, torch.cat(cols, -1))
        f = torch.cat(formula("physics_equation", 0.002, cols, [Y[:, j:j + 1] for j in range(6)]), 1).t()      # (3, N)
        w = lam * lam if mask == "square" else lam
        loss = fid + (w * f ** 2).sum() / Xr.shape[0]
        losses.append(float(loss.detach()))
        f2 = (f ** 2).detach()
        loss.backward()
        lam.grad.neg_()                                                  # ascent
        opt.step(); sched.step()
    return np.array(losses), lam.detach(), f2


def _spearman(a, b):
    ra, rb = a.reshape(-1).argsort().argsort().double(), b.reshape(-1).argsort().argsort().double()
    ra, rb = ra - ra.mean(), rb - rb.mean()
    return float((ra * rb).sum() / (ra.norm() * rb.norm()))


@pytest.mark.parametrize("mask", ["square", "linear"])
def test_trainer_self_adaptive_follows_the_fp64_loop_and_lbfgs_holds_the_weights(mask, tmp_path):
    from pinn_depthestimation_amd.trainer import PINN
    params, Xf, Tf, Xr = _trainer_data()
    l64, lam64, f2 = _sa_loop(params, Xf, Tf, Xr, mask, torch.float64)
    l32, lam32, _ = _sa_loop(params, Xf, Tf, Xr, mask, torch.float32)
    tr = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), _cfg(lbfgs_it=4), dnn=_model(params), log_every=1, checkpoint_every=0,
              log_dir=str(tmp_path), self_adaptive={"mask": mask}, lbfgs_impl="flat")
    assert tr._lam.shape == (3, N_RES) and torch.equal(tr.residual_weights(), torch.ones(3, N_RES, device="cuda"))
    tr.train_adam(ITERS)
    assert tr._folded_iters == 0 and tr.iter == ITERS
    got = np.array([h[3] for h in tr.history])
    lam = tr._lam.detach().cpu().double()
    gap_l = np.maximum.accumulate(np.abs(l32 - l64) / np.abs(l64))
    rel_l = np.abs(got - l64) / np.abs(l64)
    tol_l = np.maximum(1e-5, 4 * gap_l)
    gap_lam = float(((lam32.double() - lam64).abs() / lam64.abs()).max())
    rel_lam = float(((lam - lam64).abs() / lam64.abs()).max())
    tol_lam = max(1e-5, 4 * gap_lam)
    rho64, rho = _spearman(lam64 - 1, f2), _spearman(lam - 1, f2)
    print(f"self-adaptive {mask}: loss max rel err {rel_l.max():.2e} (worst over its bound {(rel_l / tol_l).max():.3f}; the fp32 twin's "
          f"gap {gap_l[-1]:.2e}); lambda max rel err {rel_lam:.2e} (bound {tol_lam:.2e}); lambda in [{float(lam.min()):.4f}, "
          f"{float(lam.max()):.4f}]; rank correlation of lambda - 1 with f^2: {rho:.4f} (fp64 loop {rho64:.4f})")
    assert (rel_l < tol_l).all(), (int(np.argmax(rel_l / tol_l)), rel_l.max())
    assert rel_lam < tol_lam, (rel_lam, tol_lam)
    # Ascent: nothing fell, and the points where f^2 is largest rose.  Adam normalises every multiplier's step by its own
    # gradient history, so after 20 steps all of them have risen by about 20 learning rates and the ORDER of lambda says little
    # about f^2 (the fp64 loop's rank correlation is about 0): the order is held to the fp64 loop's instead.
    top = f2.reshape(-1) >= f2.reshape(-1).quantile(0.9)
    assert float(lam.min()) >= 1.0 and float(lam.reshape(-1)[top].min()) > 1.0 + 5 * LR_W
    assert abs(rho - rho64) <= 0.02 and _spearman(lam, lam64) > 0.99, (rho, rho64, _spearman(lam, lam64))
    w_adam = tr.residual_weights().clone()
    assert torch.equal(w_adam, tr._lam * tr._lam if mask == "square" else tr._lam)
    # the flat L-BFGS stage runs and leaves lambda as Adam left it
    lam_before, loss_before = tr._lam.clone(), float(tr.last[2])
    tr.optimizer_LBFGS.step(tr.closure)
    torch.cuda.synchronize()
    assert tr.iter > ITERS and torch.equal(tr._lam, lam_before) and torch.equal(tr.residual_weights(), w_adam)
    assert np.isfinite(float(tr.last[2])) and float(tr.last[2]) <= loss_before
    tr.save_checkpoint("model_end.pth")
    saved = np.load(tmp_path / "residual_weights.npy")
    assert saved.dtype == np.float32 and np.array_equal(saved, w_adam.cpu().numpy())
    tr2 = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), _cfg(), dnn=_model(params), checkpoint_every=0, residual_weights=saved)
    assert torch.equal(tr2.residual_weights(), w_adam)
    tr.dump_predictions(str(tmp_path / "dump.mat"))
    from scipy.io import loadmat
    assert np.array_equal(loadmat(str(tmp_path / "dump.mat"))["residual_weights"], saved)


def test_trainer_zero_weights_train_as_the_other_points_alone():
    """Weight 0 on half the points against training on the other half with weight_res_loss scaled by kept / N (res_scale is
    weight / N, the normaliser the point count).  Five iterations of logged total losses: the first differs by the sums'
    rounding (2e-6), the later ones follow gradients that agree within the gradient bound, so 2e-5 relative holds them."""
    from pinn_depthestimation_amd.trainer import PINN
    params, Xf, Tf, Xr = _trainer_data()
    keep = torch.arange(N_RES) % 2 == 0
    w = keep.float()
    a = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), _cfg(), dnn=_model(params), log_every=1, checkpoint_every=0, residual_weights=w.numpy())
    a.train_adam(5)
    cfg_b = _cfg(weight_res_loss=float(keep.sum()) / N_RES)
    b = PINN(Xf.numpy(), Tf.numpy(), Xr[keep].numpy(), cfg_b, dnn=_model(params), log_every=1, checkpoint_every=0)
    b.train_adam(5)
    la, lb = np.array([h[3] for h in a.history]), np.array([h[3] for h in b.history])
    rel = np.abs(la - lb) / np.abs(lb)
    print(f"zero weights on {int((~keep).sum())} of {N_RES} points against the kept points alone: total loss max rel err {rel.max():.2e}")
    assert la.shape == lb.shape == (5,) and (rel < 2e-5).all(), rel
    assert a._folded_iters == 0
    a.set_residual_weights(None)
    assert a.residual_weights() is None and a.evaluator.point_w is None


def test_trainer_rad_importance_weights_reach_the_engine():
    from pinn_depthestimation_amd.trainer import PINN, rad_importance_weights
    params, Xf, Tf, Xr = _trainer_data()
    tr = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), _cfg(), dnn=_model(params), log_every=1, checkpoint_every=0, residual_batch=64,
              resample="rad", rad_every=100, rad_importance=True)
    tr.train_adam(5)
    torch.cuda.synchronize()
    assert tr.iter == 5 and tr._rad_at == 0 and tr._folded_iters == 0                    # one re-scoring
    want = rad_importance_weights(tr._rad_score, tr._last_idx)
    assert tr.evaluator.point_w.shape == (1, 64) and torch.equal(tr.evaluator.point_w, want)
    assert float(want.min()) > 0 and float(want.max()) != float(want.min())
    assert all(np.isfinite(h[3]) for h in tr.history)

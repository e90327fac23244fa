"""pinn_adam_loop_ext / pinn_query_adam_ext_workspace, everything that needs no GPU: the refusal table (decided before any
device work, so it answers without a device), the workspace query, the trainer's option (fold_extras_refusal, the config
key) and the NumPy restatement of the finishing kernel's multiplier step against trainer.sa_weight_grad + torch.optim.Adam
on CPU tensors — the reference tests/test_fold_ext_gpu.py holds the kernel to."""
import ctypes as C

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import NetDesc, ResidualSpec, _lib
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, ERR_INVALID, ERR_UNSUPPORTED, PREC_BF16)
from pinn_depthestimation_amd.config import load_config
from pinn_depthestimation_amd.trainer import fold_extras_refusal, sa_weight_grad
from tests import fold_ext_util as F

PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
FAKE = 0x1000      # a non-NULL address nothing dereferences: every refusal is decided before a pointer is looked at


def _pe(**kw):
    d = NetDesc(2, 6, 10, 10, (0, 1), **kw)
    return d, ResidualSpec.from_names("physics_equation", ("x", "y"), d.grad_cols, PE_OUT)


def _ns(**kw):
    d = NetDesc(3, 4, 8, 64, (0, 1, 2), **kw)
    return d, ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), d.grad_cols, ("h", "z", "u", "v"))


def _extras(kind, w_rows=3, sa_mask=0):
    ex = _lib.PinnAdamExtras()
    if "coef" in kind:
        ex.coef = ex.coef_m = ex.coef_v = ex.coef_grad = FAKE
    if "w" in kind or "sa" in kind:
        ex.point_w, ex.w_rows = FAKE, w_rows
    if "sa" in kind:
        ex.lam = ex.lam_m = ex.lam_v = ex.fields = FAKE
        ex.sa_mask = sa_mask
    return ex


def _query(desc, spec, ex, n_res=243, n_fid=12):
    lib, b = _lib.load(), C.c_int64(-1)
    rc = lib.pinn_query_adam_ext_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), None if ex is None else C.byref(ex),
                                           n_res, n_fid, C.byref(b))
    return rc, b.value, lib.pinn_last_error().decode()


def _loop(desc, spec, ex, n_iters=3, n_res=243, n_fid=12):
    """The call itself WITHOUT arrays: a refusal comes back with its code; a served request stops at the NULL arguments."""
    lib = _lib.load()
    st = _lib.PinnAdamState(None, None, 1, 0.0, 0.9, 0.999, 1e-8, 0, 0, None, None)
    rc = lib.pinn_adam_loop_ext(C.byref(desc.c_struct()), C.byref(spec.c_struct()), None, None, None, n_fid, 0, None, None, None,
                                None, n_res, None, None, None, C.byref(st), None if ex is None else C.byref(ex), n_iters, None,
                                None, None, None, 0, None)
    return rc, lib.pinn_last_error().decode()


def test_abi_version_stays_4():
    assert _lib.load().pinn_version() == 4


@pytest.mark.parametrize("kind", ["coef", "w", "sa"])
@pytest.mark.parametrize("engine,served", [(ENGINE_AUTO, True), (ENGINE_FUSED, True), (ENGINE_FUSED_TILE, True), (ENGINE_GENERIC, False),
                                           (ENGINE_WIDE, False), (ENGINE_FUSED_COOP, False), (ENGINE_FUSED_BATCH, False)])
def test_every_engine_value(kind, engine, served):
    for mk in (_pe, _ns):
        desc, spec = mk(engine=engine)
        ex = _extras(kind)
        rc, b, _ = _query(desc, spec, ex)
        rcl, msg = _loop(desc, spec, ex)
        if served:
            assert rc == 0 and b > 0
            assert rcl == ERR_INVALID and "bad arguments" in msg          # past every refusal, stopped at the NULL arrays
        else:
            assert rc == ERR_UNSUPPORTED and rcl == ERR_UNSUPPORTED, (rc, rcl)


@pytest.mark.parametrize("kind", ["coef", "w", "sa"])
def test_descriptor_refusals(kind):
    ex = _extras(kind)
    for what, kw, word in (("bf16", dict(precision=PREC_BF16), "bf16"), ("dropout", dict(dropout_p=0.1), "dropout"),
                           ("leaky", dict(activation=ACT_LEAKY_RELU), "LeakyReLU")):
        desc, spec = _pe(**kw)
        rc, _, msg = _query(desc, spec, ex)
        assert rc == ERR_UNSUPPORTED and word in msg, (what, rc, msg)
        assert _loop(desc, spec, ex)[0] == ERR_UNSUPPORTED, what
    d65 = NetDesc(2, 6, 3, 65, (0, 1))
    s65 = ResidualSpec.from_names("physics_equation", ("x", "y"), d65.grad_cols, PE_OUT)
    rc, _, msg = _query(d65, s65, ex)
    assert rc == ERR_UNSUPPORTED and "width" in msg
    assert _loop(d65, s65, ex)[0] == ERR_UNSUPPORTED
    desc, _ = _pe()
    pec = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, PE_OUT, corrected=True)
    rc, _, msg = _query(desc, pec, ex)
    assert rc == ERR_UNSUPPORTED and "corrected" in msg
    rcl, msg = _loop(desc, pec, ex)
    assert rcl == ERR_UNSUPPORTED and "corrected" in msg
    # k must be the residual's directions: physics_equation on a network that differentiates three inputs
    d3 = NetDesc(3, 6, 2, 10, (0, 1, 2))
    s3 = ResidualSpec.from_names("physics_equation", ("t", "x", "y"), d3.grad_cols, PE_OUT)
    assert _query(d3, s3, ex)[0] == ERR_UNSUPPORTED and _loop(d3, s3, ex)[0] == ERR_UNSUPPORTED


def test_both_groups_neither_group_and_bad_rows():
    desc, spec = _pe()
    rc, _, msg = _query(desc, spec, _extras("coef+sa"))
    assert rc == ERR_UNSUPPORTED and "no kernel carries both" in msg
    rcl, msg = _loop(desc, spec, _extras("coef+w"))
    assert rcl == ERR_UNSUPPORTED and "no kernel carries both" in msg
    for ex in (_lib.PinnAdamExtras(), None):
        rc, _, msg = _query(desc, spec, ex)
        assert rc == ERR_INVALID and "pinn_adam_loop" in msg
        assert _loop(desc, spec, ex)[0] == ERR_INVALID
    for rows in (0, 2, 4):
        rc, _, msg = _query(desc, spec, _extras("w", w_rows=rows))
        assert rc == ERR_INVALID and "w_rows" in msg, rows
        assert _loop(desc, spec, _extras("sa", w_rows=rows))[0] == ERR_INVALID
    assert _query(desc, spec, _extras("w", w_rows=1))[0] == 0 and _query(desc, spec, _extras("w", w_rows=3))[0] == 0
    assert _query(desc, spec, _extras("sa", sa_mask=2))[0] == ERR_INVALID
    assert _query(desc, spec, _extras("w"), n_res=0)[0] == ERR_INVALID and _query(desc, spec, _extras("w"), n_fid=-1)[0] == ERR_INVALID


def test_continuity_residuals():
    d = NetDesc(2, 3, 100, 20, (0, 1))
    for name, n_w in (("continuity_only", 2), ("continuity_ftemp", 1)):
        spec = ResidualSpec.from_names(name, ("x", "y"), d.grad_cols, ("U", "V", "h"))
        rc, _, msg = _query(d, spec, _extras("coef"))
        assert rc == ERR_UNSUPPORTED and "no coefficient" in msg
        rcl, msg = _loop(d, spec, _extras("coef"))
        assert rcl == ERR_UNSUPPORTED and "no coefficient" in msg
        assert _query(d, spec, _extras("sa", w_rows=n_w))[0] == 0 and _query(d, spec, _extras("w", w_rows=1))[0] == 0
        if n_w != 3:
            assert _query(d, spec, _extras("w", w_rows=3))[0] == ERR_INVALID


def test_zero_iterations_is_ok_and_negative_is_invalid():
    desc, spec = _pe()
    assert _loop(desc, spec, _extras("coef"), n_iters=0)[0] == 0
    assert _loop(desc, spec, _extras("sa"), n_iters=0)[0] == 0
    assert _loop(desc, spec, _extras("coef"), n_iters=-1)[0] == ERR_INVALID
    # ... but a refusal is a refusal whatever n_iters
    dg, sg = _pe(engine=ENGINE_GENERIC)
    assert _loop(dg, sg, _extras("coef"), n_iters=0)[0] == ERR_UNSUPPORTED


@pytest.mark.parametrize("mk,kind", [(_pe, "coef"), (_pe, "sa"), (_ns, "coef"), (_ns, "w")])
def test_query_grows_and_covers_the_single_entries(mk, kind):
    lib = _lib.load()
    desc, spec = mk()
    ex = _extras(kind)
    single = lib.pinn_query_residual_coef_workspace if kind == "coef" else lib.pinn_query_residual_weighted_workspace
    prev = 0
    for n_res in (1, 243, 4099, 1 << 20):
        rc, b, _ = _query(desc, spec, ex, n_res=n_res, n_fid=12)
        s = C.c_int64()
        assert rc == 0 and single(C.byref(desc.c_struct()), C.byref(spec.c_struct()), n_res, C.byref(s)) == 0
        assert b >= s.value and b >= prev, (n_res, b, s.value, prev)
        prev = b
    assert prev > _query(desc, spec, ex, n_res=1)[1]
    # ... with the fidelity points: never smaller, larger once they outnumber the collocation points; and enough for a
    # K1 = 1 pass on them (pinn_query_workspace answers for every call on the descriptor)
    b0 = _query(desc, spec, ex, n_res=243, n_fid=0)[1]
    b1 = _query(desc, spec, ex, n_res=243, n_fid=243)[1]
    b2 = _query(desc, spec, ex, n_res=243, n_fid=1 << 16)[1]
    assert b0 <= b1 <= b2 and b2 > b0
    q = C.c_int64()
    assert lib.pinn_query_workspace(C.byref(desc.c_struct()), 1 << 16, C.byref(q)) == 0 and b2 >= q.value


def test_fold_extras_refusal():
    assert fold_extras_refusal() is None
    assert fold_extras_refusal(False, coefficients=True, residual_batch=64) is None          # the option is off: nothing to decide
    assert fold_extras_refusal(True) is None                                                 # neither coefficients nor weights
    assert fold_extras_refusal(True, coefficients=True) is None
    assert fold_extras_refusal(True, weighted=True) is None
    for kw, word in ((dict(residual_batch=64), "residual_batch"), (dict(resample="rad", residual_batch=64), "rad"),
                     (dict(rad_importance=True), "rad"), (dict(dropout_rate=0.1), "dropout"), (dict(reducer_active=True), "parallel"),
                     (dict(eddy_viscosity=0.1), "eddy_viscosity"), (dict(custom_evaluator=True), "custom"),
                     (dict(fold_adam=False), "fold_adam")):
        why = fold_extras_refusal(True, weighted=True, **kw)
        assert why and word in why, (kw, why)
        assert fold_extras_refusal(True, coefficients=True, **kw)


def test_config_key():
    cfg = {
        "layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0, "init_type": "xavier"},
        "adam_optimizer": {"max_it": 20, "learning_rate": 1e-3, "scheduler_step_size": 7, "scheduler_gamma": 0.8},
        "lbfgs_optimizer": {"max_it": 0, "learning_rate": 1, "max_evaluation": 12, "history_size": 10,
                            "tolerance_grad": 1e-9, "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": list(PE_OUT), "training_points": 12},
        "data_residual": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}}, "outputs": list(PE_OUT)},
    }
    assert load_config(cfg).fold_extras is False
    cfg["adam_optimizer"]["fold_extras"] = True
    assert load_config(cfg).fold_extras is True


@pytest.mark.parametrize("mask", ["square", "linear"])
@pytest.mark.parametrize("rows", [1, 3])
def test_multiplier_step_restated_in_numpy_is_sa_weight_grad_plus_torch_adam(mask, rows):
    """Five steps with learning-rate changes; before every step the restatement takes torch's own state (lambda, exp_avg,
    exp_avg_sq), so each step is compared on identical inputs, ELEMENT BY ELEMENT.
    The gradient: exact products in a fixed order for a row per term — bit for bit; a shared row adds three terms in torch's
    order, held to 2 eps of each entry.
    Adam: torch's CPU kernels form each of the three updates as one fused operation (lerp m + w (g - m), addcmul
    v b2 + (w2 g) g, addcdiv p - s (m / d)) whose last product may be contracted into the sum; the restatement — and the
    kernel, with contraction off — rounds the product first.  One rounding more or less moves a result by at most one unit in
    its last place, which is at most eps |x|; lambda also reads the new m and v, whose one-unit difference reaches it scaled by
    the learning rate.  So every entry of lambda, m and v is held to 2 eps |entry|, in float32 and in float64.  Equality with
    torch's CPU kernels is NOT claimed (measured: up to 1.0 eps |entry|).  At step 1 the moments start from zero, a contracted
    product added to zero rounds once either way, and m and v are bit for bit."""
    n = 517
    g = torch.Generator().manual_seed(5 + rows)
    scale = torch.tensor([0.7, 1.3, 0.9]) / n
    for dtype in (torch.float32, torch.float64):
        eps = float(np.finfo(np.float32 if dtype == torch.float32 else np.float64).eps)
        lam = (0.5 + torch.rand(rows, n, generator=g)).to(dtype)
        ref = lam.clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=1e-2, maximize=False)
        worst = 0.0
        for step in (1, 2, 3, 4, 5):
            lr = 1e-2 * 0.8 ** (step // 3)
            fields = (torch.randn(3, n, generator=g) * 3).to(dtype)
            for grp in opt.param_groups:
                grp["lr"] = lr
            ref.grad = sa_weight_grad(ref.detach(), fields, scale.to(dtype), mask).contiguous()
            gn = F.sa_grad(ref.detach().numpy(), fields.numpy(), scale.to(dtype).numpy(), mask)
            if rows == 3:
                assert np.array_equal(gn, ref.grad.numpy())
            else:
                assert (np.abs(gn - ref.grad.numpy()) <= 2 * eps * np.abs(ref.grad.numpy())).all()
            st = opt.state[ref]
            nl = ref.detach().numpy().copy()
            nm = st["exp_avg"].numpy().copy() if step > 1 else np.zeros_like(nl)
            nv = st["exp_avg_sq"].numpy().copy() if step > 1 else np.zeros_like(nl)
            before = nl.copy()
            opt.step()
            st = opt.state[ref]
            nl, nm, nv, w = F.multiplier_step(nl, nm, nv, fields.numpy(), scale.to(dtype).numpy(), mask, lr, step)
            for name, got, want in (("lambda", nl, ref.detach().numpy()), ("exp_avg", nm, st["exp_avg"].numpy()),
                                    ("exp_avg_sq", nv, st["exp_avg_sq"].numpy())):
                assert got.dtype == want.dtype
                ratio = float((np.abs(got - want) / np.maximum(eps * np.abs(want), np.finfo(want.dtype).tiny)).max())
                worst = max(worst, ratio)
                assert (np.abs(got - want) <= 2 * eps * np.abs(want)).all(), (name, step, ratio)
                if step == 1 and name != "lambda":
                    assert np.array_equal(got, want), name
            assert np.array_equal(w, nl * nl if mask == "square" else nl)
            assert (nl >= before).all()      # ascent: the gradient Adam descends along is never positive
        print(f"{mask} rows={rows} {dtype}: worst |difference| / (eps |entry|) over five steps {worst:.2f} (bound 2)")

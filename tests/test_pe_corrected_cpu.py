"""The corrected radiation-stress residual (pinn_residual_spec.flags bit 0 on physics_equation), everything that needs no
GPU: the host evaluation pinn_pe_corrected_point — the very functions the kernels call — against torch autograd in float64
over the Python formula, the plumbing of the flag, the refusals (made before any device work) and the trainer's keyword."""
import ctypes as C

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import NetDesc, ResidualSpec, _lib, engine, physics
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_GENERIC, ENGINE_WIDE, ERR_UNSUPPORTED,
                                           ERR_WORKSPACE, PREC_BF16, PinnError)
from tests.pe_corrected_util import ROLES, pec_fields, pec_loss

PE_IN, PE_OUT = ("x", "y"), ROLES
ERR_LAUNCH = -4      # PINN_ERR_LAUNCH (include/pinn_hip.h): a device call failed — never the answer to a refused request


def _spec(desc, corrected=True, inputs=PE_IN):
    return ResidualSpec.from_names("physics_equation", inputs, desc.grad_cols, PE_OUT, corrected=corrected)


# ---- pinn_pe_corrected_point against fp64 autograd over the formula ----------------------------------------------------
def _point(v, scale=None, want_g=True, g_fill=None):
    """One call: v (18,) float32 -> (fields (3,), g (18,))."""
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    v = np.ascontiguousarray(v, dtype=np.float32)
    f = np.zeros(3, dtype=np.float32)
    g = np.full(18, 0.0 if g_fill is None else g_fill, dtype=np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    rc = lib.pinn_pe_corrected_point(v.ctypes.data_as(fp), None if sc is None else sc.ctypes.data_as(fp), f.ctypes.data_as(fp),
                                     g.ctypes.data_as(fp) if want_g else None)
    assert rc == 0, lib.pinn_last_error()
    return f, g


def _autograd_reference(V, scale):
    """V (n, 18) float32 jets -> fp64 fields (n, 3) and adjoint (n, 18) of sum_t scale[t] field_t^2, by torch autograd over
    the Python formula: each role is the affine function of (x, y) whose value and gradient at the point are the jet's."""
    V64 = torch.tensor(V, dtype=torch.float64).reshape(-1, 3, 6).requires_grad_(True)
    n = V64.shape[0]
    x = torch.zeros(n, 1, dtype=torch.float64, requires_grad=True)
    y = torch.zeros(n, 1, dtype=torch.float64, requires_grad=True)
    outs = [V64[:, 0, r:r + 1] + V64[:, 1, r:r + 1] * x + V64[:, 2, r:r + 1] * y for r in range(6)]
    f = torch.cat(pec_fields(x, y, *outs), dim=1)
    obj = (f ** 2 * torch.tensor(scale, dtype=torch.float64)).sum()
    (g,) = torch.autograd.grad(obj, V64)
    return f.detach().numpy(), g.reshape(n, 18).numpy()


def _jets(n, seed, kh=None):
    """Random jets around the conditioned operating point (h ~ 2, eta ~ 0.2, Hrms ~ 0.5, k ~ 1, gradients O(0.3)); with
    `kh` (n,) the wave number is set so that k h takes those values."""
    r = np.random.default_rng(seed)
    V = np.zeros((n, 3, 6))
    V[:, 0, 0] = r.uniform(1.6, 2.4, n)            # h
    V[:, 0, 1:3] = r.uniform(-0.5, 0.5, (n, 2))    # U, V
    V[:, 0, 3] = r.uniform(0.1, 0.3, n)            # eta
    V[:, 0, 4] = r.uniform(0.3, 0.7, n)            # Hrms
    V[:, 0, 5] = r.uniform(0.9, 1.1, n) if kh is None else kh / V[:, 0, 0]
    V[:, 1:, :] = r.uniform(-0.3, 0.3, (n, 2, 6))
    return V.reshape(n, 18).astype(np.float32)


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def _host_all(V, scale):
    F, G = np.zeros((len(V), 3), np.float32), np.zeros((len(V), 18), np.float32)
    for i, v in enumerate(V):
        F[i], G[i] = _point(v, scale)
    return F, G


SCALE = (0.7, 1.3, 0.9)


def test_point_matches_fp64_autograd_in_the_conditioned_range():
    V = _jets(4000, 11)
    F, G = _host_all(V, SCALE)
    Fr, Gr = _autograd_reference(V, SCALE)
    ef, eg = _rel_l2(F, Fr), _rel_l2(G, Gr)
    print(f"conditioned: fields rel_l2 {ef:.2e}, adjoint rel_l2 {eg:.2e}")
    assert ef < 2e-6 and eg < 2e-5


def test_point_matches_fp64_autograd_for_kh_from_1e_minus_3_to_40_both_signs():
    r = np.random.default_rng(12)
    kh = np.exp(r.uniform(np.log(1e-3), np.log(40.0), 4000)) * r.choice([-1.0, 1.0], 4000)
    V = _jets(4000, 13, kh)
    F, G = _host_all(V, SCALE)
    Fr, Gr = _autograd_reference(V, SCALE)
    ef, eg = _rel_l2(F, Fr), _rel_l2(G, Gr)
    print(f"|kh| in [1e-3, 40]: fields rel_l2 {ef:.2e}, adjoint rel_l2 {eg:.2e}")
    assert ef < 2e-6 and eg < 2e-5
    # ... and point by point around the series / closed-form switch at |kh| = 1/4 (no jump there)
    near = np.abs(np.abs(kh) - 0.25) < 0.1
    assert near.sum() > 50
    assert _rel_l2(F[near], Fr[near]) < 2e-6 and _rel_l2(G[near], Gr[near]) < 2e-5


@pytest.mark.parametrize("kh", [0.0, 60.0, -60.0, 100.0, -100.0])
def test_point_is_finite_at_kh_zero_and_where_sinh_overflows(kh):
    V = _jets(1, 14, np.array([kh]))
    f, g = _point(V[0], SCALE)
    assert np.isfinite(f).all() and np.isfinite(g).all(), (kh, f, g)
    if kh == 0.0:   # the limit n = 1/2, n' = 0: Sxx_x = E_x 3/2, Syy_y = E_y / 2
        v = V[0].astype(np.float64).reshape(3, 6)
        D, CE = 1.0 / (1025 * (v[0, 3] + v[0, 0])), 1025 * 9.81 / 8
        fx = v[0, 1] * v[1, 1] + v[0, 2] * v[2, 1] + 9.81 * v[1, 3] + D * (1025 * 0.002 * v[0, 1] * abs(v[0, 1]) + 2 * CE * v[0, 4] * v[1, 4] * 1.5)
        assert abs(f[1] - fx) < 2e-6 * abs(fx)


def test_point_without_scale_or_g_forms_the_fields_only():
    V = _jets(1, 15)
    f0, _ = _point(V[0], SCALE)
    f1, g1 = _point(V[0], None, g_fill=7.0)
    assert np.array_equal(f0, f1) and np.all(g1 == 7.0)          # g untouched
    f2, _ = _point(V[0], SCALE, want_g=False)
    assert np.array_equal(f0, f2)


def test_the_test_formula_is_the_packages():
    """pe_corrected_util.pec_loss restates physics.physics_equation(corrected=True) (it needs the fields apart)."""
    V = torch.tensor(_jets(50, 16), dtype=torch.float64).reshape(-1, 3, 6)
    x = torch.zeros(50, 1, dtype=torch.float64, requires_grad=True)
    y = torch.zeros(50, 1, dtype=torch.float64, requires_grad=True)
    outs = [V[:, 0, r:r + 1] + V[:, 1, r:r + 1] * x + V[:, 2, r:r + 1] * y for r in range(6)]
    a = physics.physics_equation(x, y, *outs, corrected=True)
    assert float(a.detach()) == pytest.approx(float(pec_loss(x, y, *outs).detach()), rel=1e-14)
    assert float(physics.physics_equation_corrected(x, y, *outs).detach()) == float(a.detach())      # plain tensors: the formula
    assert float(a.detach()) != pytest.approx(float(physics.physics_equation(x, y, *outs).detach()), rel=1e-3)


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_flag_and_tables():
    d = NetDesc(2, 6, 10, 10, (0, 1))
    assert _spec(d, False).c_struct().flags == 0 and ResidualSpec("physics_equation", (0, 1, 2, 3, 4, 5), (0, 1)).c_struct().flags == 0
    s = _spec(d, True)
    assert s.corrected and s.c_struct().flags == 1 and s.c_struct().residual_id == _lib.RES_PHYSICS_EQUATION
    assert s.n_terms == 3 and s.n_fields == 3
    assert sorted(engine.RESIDUAL_ROLES) == ["Navier_Stokes", "continuity_ftemp", "continuity_only", "physics_equation"]
    assert _lib.RES_TERMS == {1: 3, 2: 3, 3: 1, 4: 3} and _lib.RES_FIELDS == {1: 3, 2: 3, 3: 2, 4: 2}
    with pytest.raises(PinnError, match="corrected"):
        ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), (0, 1, 2), ("h", "z", "u", "v"), corrected=True)
    lib = _lib.load()
    assert "pinn_pe_corrected_point" in _lib.exported_symbols() and lib.pinn_pe_corrected_point.restype is C.c_int32
    assert lib.pinn_version() == _lib.ABI_VERSION == 4


def test_the_internal_residual_id_is_not_a_public_one():
    d = NetDesc(2, 6, 10, 10, (0, 1))
    s = _spec(d).c_struct(); s.residual_id = 5
    need = C.c_int64()
    lib = _lib.load()
    assert lib.pinn_query_fields_workspace(C.byref(d.c_struct()), C.byref(s), 16, C.byref(need)) == _lib.ERR_INVALID
    assert "residual_id" in lib.pinn_last_error().decode()


# ---- refusals, before any device work: fake pointers -------------------------------------------------------------------
_P = C.c_void_p(0x1000)


def _loss_calls(desc, spec, workspace=True):
    """Every loss entry that takes a spec, with fake non-NULL pointers: (name, rc, message).  For requests that are REFUSED
    only: a request the engine serves must come with workspace=False (ws = NULL, ws_bytes = 0), which every engine turns
    down with PINN_ERR_WORKSPACE before its first device call — with a workspace "size" of 2^40 such a request passes
    validation and packs, launches and memsets on the fake addresses.  N = 64 with n_res = 48 (or both terms on every
    point): no entry zeroes col_sums ahead of that check, which the n_res == N forms do."""
    lib = _lib.load()
    d, s = desc.c_struct(), spec.c_struct()
    oc = (C.c_int32 * 1)(0)
    st = _lib.PinnAdamState(_P, _P, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None)
    lr = (C.c_double * 2)(1e-3, 1e-3)
    ws, big = (_P, 1 << 40) if workspace else (None, 0)
    calls = [
        ("pinn_residual_loss", lambda: lib.pinn_residual_loss(C.byref(d), C.byref(s), _P, _P, 64, _P, ws, big, None)),
        ("pinn_residual_loss_grad", lambda: lib.pinn_residual_loss_grad(C.byref(d), C.byref(s), _P, _P, _P, 64, _P, _P, ws, big, None)),
        ("pinn_residual_mse_loss_grad", lambda: lib.pinn_residual_mse_loss_grad(C.byref(d), C.byref(s), _P, _P, 1, oc, _P, _P, _P, 64, _P, _P,
                                                                                _P, ws, big, None)),
        ("pinn_residual_mse_split_loss_grad", lambda: lib.pinn_residual_mse_split_loss_grad(C.byref(d), C.byref(s), _P, _P, 1, oc, _P, _P, _P, 64,
                                                                                            48, _P, _P, _P, ws, big, None)),
        ("pinn_loss_grad_adam_step", lambda: lib.pinn_loss_grad_adam_step(C.byref(d), C.byref(s), _P, _P, 1, oc, _P, _P, _P, 64, 48, _P, _P, _P,
                                                                          C.byref(st), ws, big, None)),
        ("pinn_adam_loop", lambda: lib.pinn_adam_loop(C.byref(d), C.byref(s), _P, _P, 1, oc, _P, _P, _P, 64, 48, _P, _P, _P, C.byref(st), 2, lr,
                                                      ws, big, None)),
    ]
    return [(name, fn(), lib.pinn_last_error().decode()) for name, fn in calls]


def _fields_query(desc, spec):
    lib = _lib.load()
    need = C.c_int64(-1)
    rc = lib.pinn_query_fields_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), 64, C.byref(need))
    return rc, need.value, lib.pinn_last_error().decode()


K3 = NetDesc(3, 6, 3, 20, (0, 1, 2), engine=ENGINE_FUSED)
REFUSED = {
    "width 100, AUTO": NetDesc(2, 6, 3, 100, (0, 1)),
    "width 100, WIDE": NetDesc(2, 6, 3, 100, (0, 1), engine=ENGINE_WIDE),
    "bf16": NetDesc(2, 6, 3, 128, (0, 1), precision=PREC_BF16),
    "LeakyReLU, FUSED": NetDesc(2, 6, 3, 20, (0, 1), activation=ACT_LEAKY_RELU, engine=ENGINE_FUSED),
    "k = 3, FUSED": K3,
}


def _spec_for(desc):
    return _spec(desc, True, ("x", "y", "t") if desc.k == 3 else PE_IN)


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_loss_entries_refuse_with_the_reason(case):
    desc = REFUSED[case]
    for name, rc, msg in _loss_calls(desc, _spec_for(desc)):
        assert rc == ERR_UNSUPPORTED and "corrected" in msg, (case, name, rc, msg)
    if "GENERIC" not in case:
        assert "GENERIC" in msg
    # the plain residual on the same descriptor is not refused for that reason.  Most of these descriptors SERVE it, so
    # the calls carry no workspace: they stop at the workspace check (or at another refusal), ahead of any device work
    plain = ResidualSpec.from_names("physics_equation", ("x", "y", "t") if desc.k == 3 else PE_IN, desc.grad_cols, PE_OUT)
    for name, rc, msg in _loss_calls(desc, plain, workspace=False):
        assert rc in (ERR_WORKSPACE, ERR_UNSUPPORTED), (case, name, rc, msg)
        assert rc != ERR_LAUNCH, (case, name, msg)
        assert "corrected" not in msg, (case, name, rc, msg)


@pytest.mark.parametrize("case", ["LeakyReLU, FUSED", "k = 3, FUSED"])
def test_fields_query_refuses_what_the_fused_engine_does_not_serve(case):
    desc = REFUSED[case]
    rc, _, msg = _fields_query(desc, _spec_for(desc))
    assert rc == ERR_UNSUPPORTED and "corrected" in msg, (rc, msg)


@pytest.mark.parametrize("case", sorted(c for c in REFUSED if "k = 3" not in c))
def test_fields_query_passes_on_the_generic_engine(case):
    """(a k = 3 descriptor stays refused there as well: pinn_residual_fields needs k = the residual's two directions)"""
    desc = REFUSED[case].with_(engine=ENGINE_GENERIC, precision=0)
    rc, need, msg = _fields_query(desc, _spec_for(desc))
    assert rc == 0 and need > 0, msg


def test_fields_query_answers_for_either_path():
    d = NetDesc(2, 6, 10, 10, (0, 1))
    tile = _fields_query(d, _spec(d))                                     # AUTO, tanh: the tile kernel's field instances
    staged = _fields_query(d.with_(engine=ENGINE_GENERIC), _spec(d))
    assert tile[0] == 0 and staged[0] == 0 and staged[1] > tile[1] > 0
    assert tile[1] == _fields_query(d, _spec(d, False))[1]
    leaky = d.with_(activation=ACT_LEAKY_RELU)                            # AUTO, LeakyReLU: staged on the fused forward jet
    lk = _fields_query(leaky, _spec(leaky))
    assert lk[0] == 0 and lk[1] > _fields_query(leaky, _spec(leaky, False))[1]
    wide = NetDesc(2, 6, 3, 100, (0, 1))                                  # the staged path serves the other engines too
    assert _fields_query(wide, _spec(wide))[0] == 0


# ---- trainer ---------------------------------------------------------------------------------------------------------
def _cfg(outputs, **loss):
    return {"layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": len(outputs)},
            "adam_optimizer": {"max_it": 2, "learning_rate": 1e-3, "scheduler_step_size": 10000, "scheduler_gamma": 0.8},
            "lbfgs_optimizer": {"max_it": 0}, "loss": dict({"weight_fid_loss": 1, "weight_res_loss": 1}, **loss),
            "data_fidelity": {"inputs": ["x", "y"], "outputs": []},
            "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"}, "outputs": list(outputs)}}


class _Stub:
    def __call__(self, theta, Xf, Tf, fid_scale, Xr, res_scale, grad, fid_sums, res_sums):
        fid_sums.zero_(); res_sums.fill_(1.0)

    def adam_step(self, theta, grad, m, v, step, lr):
        pass


def _pinn(cfg, **kw):
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.trainer import PINN
    L = cfg["layers"]
    layers = [2] + [L["hidden_width"]] * L["hidden_layers"] + [L["output_features"]]
    return PINN(None, None, np.zeros((32, 2), np.float32), cfg, device="cpu", dnn=DNN(layers, 0.0, "xavier"), checkpoint_every=0,
                evaluator=_Stub(), **kw)


def test_trainer_keyword_and_config_key():
    assert not _pinn(_cfg(ROLES)).spec.corrected
    assert _pinn(_cfg(ROLES), corrected=True).spec.corrected
    tr = _pinn(_cfg(ROLES, corrected_radiation_stress=True))
    assert tr.corrected and tr.spec.corrected and tr.spec.c_struct().flags == 1
    assert not _pinn(_cfg(ROLES, corrected_radiation_stress=False)).spec.corrected
    with pytest.raises(PinnError, match="corrected"):
        _pinn(_cfg(("U", "V", "h")), corrected=True, residual="continuity_ftemp")
    with pytest.raises(PinnError, match="corrected"):
        _pinn(_cfg(("U", "V", "h"), corrected_radiation_stress=True))

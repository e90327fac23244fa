"""The lateral-mixing term -nu lap(U) on the second-order jets, everything that needs no GPU: the host evaluation
pinn_residual2_point — the very functions k2_residual calls — against torch autograd in float64 over the Python formula
(tests/residual2_util.formula), the refusals of pinn_residual2_loss_grad and its workspace query (made before any device
work), the plumbing of nu through ResidualSpec, Engine, the trainer and the tester."""
import ctypes as C

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, _lib
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE, ENGINE_GENERIC,
                                           ENGINE_WIDE, ERR_INVALID, ERR_UNSUPPORTED, PREC_BF16, PinnError)
from tests.residual2_util import NS_IN, NS_OUT, PE_IN, PE_OUT, formula
from tests.test_pe_corrected_cpu import _jets as pe_jets, _point as pec_point

FP = C.POINTER(C.c_float)
SCALE = (0.7, 1.3, 0.9)
CASES = {"NS": ("Navier_Stokes", False), "PE": ("physics_equation", False), "PEC": ("physics_equation", True)}
SHAPE = {"Navier_Stokes": (4, 3, 1, 2), "physics_equation": (6, 2, 0, 1)}     # roles, directions, direction role of x, of y
MOM = {"Navier_Stokes": (2, 3), "physics_equation": (1, 2)}                   # roles of the two momentum unknowns


def _ns_jets(n, seed):
    """The conditioned range of test_pe_corrected_cpu._jets on Navier_Stokes' roles: h ~ 2, z ~ 0.2, u, v in +-0.5,
    derivatives O(0.3)."""
    r = np.random.default_rng(seed)
    V = np.zeros((n, 4, 4))
    V[:, 0, 0] = r.uniform(1.6, 2.4, n)
    V[:, 0, 1] = r.uniform(0.1, 0.3, n)
    V[:, 0, 2:4] = r.uniform(-0.5, 0.5, (n, 2))
    V[:, 1:, :] = r.uniform(-0.3, 0.3, (n, 3, 4))
    return V.reshape(n, 16).astype(np.float32)


def _jets(name, n, seed):
    V = _ns_jets(n, seed) if name == "Navier_Stokes" else pe_jets(n, seed)
    lap = np.random.default_rng(seed + 100).uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    return V, lap


def _point(name, corrected, nu, v, lap, scale=SCALE, want_g=True, fill=None):
    """One call: -> (rc, fields (3,), g (len(v),), glap (2,))."""
    lib = _lib.load()
    rid = _lib.RES_NAVIER_STOKES if name == "Navier_Stokes" else _lib.RES_PHYSICS_EQUATION
    v = np.ascontiguousarray(v, dtype=np.float32)
    lap = np.ascontiguousarray(lap, dtype=np.float32)
    f = np.zeros(3, np.float32)
    g = np.full(len(v), 0.0 if fill is None else fill, np.float32)
    gl = np.full(2, 0.0 if fill is None else fill, np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    rc = lib.pinn_residual2_point(rid, 1 if corrected else 0, C.c_float(nu), v.ctypes.data_as(FP), lap.ctypes.data_as(FP),
                                  None if sc is None else sc.ctypes.data_as(FP), f.ctypes.data_as(FP),
                                  g.ctypes.data_as(FP) if want_g else None, gl.ctypes.data_as(FP) if want_g else None)
    return rc, f, g, gl


def _host_all(name, corrected, nu, V, LAP):
    F, G, GL = np.zeros((len(V), 3), np.float32), np.zeros(V.shape, np.float32), np.zeros((len(V), 2), np.float32)
    for i in range(len(V)):
        rc, F[i], G[i], GL[i] = _point(name, corrected, nu, V[i], LAP[i])
        assert rc == 0
    return F, G, GL


def _autograd_reference(name, corrected, nu, V, LAP, scale=SCALE):
    """fp64 fields (n, 3), adjoint of the first-order jet (n, .) and of the Laplacians (n, 2) of sum_t scale[t] field_t^2:
    each role is the quadratic in (t, x, y) whose value, gradient and Hessian diagonal at the origin are the jet's (the
    Laplacian of a momentum role split between xx and yy at random; the other roles' second derivatives do not enter)."""
    nr, nd, dx, dy = SHAPE[name]
    n = len(V)
    V64 = torch.tensor(V, dtype=torch.float64).reshape(n, 1 + nd, nr).requires_grad_(True)
    L64 = torch.tensor(LAP, dtype=torch.float64).requires_grad_(True)
    split = torch.rand(n, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    ins = [torch.zeros(n, 1, dtype=torch.float64, requires_grad=True) for _ in range(nd)]
    outs = []
    for r in range(nr):
        a = V64[:, 0, r:r + 1]
        for d in range(nd):
            a = a + V64[:, 1 + d, r:r + 1] * ins[d]
        if r in MOM[name]:
            L = L64[:, MOM[name].index(r):MOM[name].index(r) + 1]
            a = a + 0.5 * L * (split * ins[dx] ** 2 + (1 - split) * ins[dy] ** 2)
        outs.append(a)
    f = torch.cat(formula(name, corrected, nu, ins, outs), dim=1)
    obj = (f ** 2 * torch.tensor(scale, dtype=torch.float64)).sum()
    g, gl = torch.autograd.grad(obj, (V64, L64))
    return f.detach().numpy(), g.reshape(n, -1).numpy(), gl.numpy()


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("nu", [0.0, 0.05, 1.0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_point_matches_fp64_autograd(case, nu):
    name, corrected = CASES[case]
    V, LAP = _jets(name, 4000, 21)
    F, G, GL = _host_all(name, corrected, nu, V, LAP)
    Fr, Gr, GLr = _autograd_reference(name, corrected, nu, V, LAP)
    ef = _rel_l2(F, Fr)
    eg = _rel_l2(np.concatenate([G, GL], 1), np.concatenate([Gr, GLr], 1))
    print(f"{case} nu={nu}: fields rel_l2 {ef:.2e}, adjoint rel_l2 {eg:.2e}")
    assert ef < 2e-6 and eg < 2e-5
    if nu == 0.0:
        assert not GL.any() and not GLr.any()
    else:
        assert _rel_l2(GL, GLr) < 2e-5


def test_nu_zero_is_the_first_order_host_entry_bit_for_bit():
    V, LAP = _jets("physics_equation", 500, 22)
    for v, lap in zip(V, LAP):
        f0, g0 = pec_point(v, SCALE)
        rc, f, g, gl = _point("physics_equation", True, 0.0, v, lap)
        assert rc == 0 and np.array_equal(f0.view(np.int32), f.view(np.int32)) and np.array_equal(g0.view(np.int32), g.view(np.int32))
        assert not gl.any()


def test_point_without_adjoint_arguments_forms_the_fields_only():
    V, LAP = _jets("Navier_Stokes", 1, 23)
    _, f0, _, _ = _point("Navier_Stokes", False, 0.3, V[0], LAP[0])
    rc, f1, g1, gl1 = _point("Navier_Stokes", False, 0.3, V[0], LAP[0], scale=None, fill=7.0)
    assert rc == 0 and np.array_equal(f0, f1) and np.all(g1 == 7.0) and np.all(gl1 == 7.0)
    rc, f2, _, _ = _point("Navier_Stokes", False, 0.3, V[0], LAP[0], want_g=False)
    assert rc == 0 and np.array_equal(f0, f2)


def test_point_refusals():
    lib = _lib.load()
    V, LAP = _jets("Navier_Stokes", 1, 24)
    for bad in (-0.1, float("nan"), float("inf")):
        assert _point("Navier_Stokes", False, bad, V[0], LAP[0])[0] == ERR_INVALID
        assert "nu" in lib.pinn_last_error().decode()
    f = np.zeros(3, np.float32)
    for rid in (_lib.RES_CONTINUITY_FTEMP, _lib.RES_CONTINUITY_ONLY):
        rc = lib.pinn_residual2_point(rid, 0, C.c_float(0.1), V[0].ctypes.data_as(FP), LAP[0].ctypes.data_as(FP), None, f.ctypes.data_as(FP),
                                      None, None)
        assert rc == ERR_UNSUPPORTED and "no second-order term" in lib.pinn_last_error().decode()
    assert lib.pinn_residual2_point(9, 0, C.c_float(0.1), V[0].ctypes.data_as(FP), LAP[0].ctypes.data_as(FP), None, f.ctypes.data_as(FP),
                                    None, None) == ERR_INVALID


# ---- refusals of the call and the query, before any device work: fake pointers ----------------------------------------
_P = C.c_void_p(0x1000)
NS = NetDesc(3, 4, 8, 64, (0, 1, 2))
PE = NetDesc(2, 6, 10, 10, (0, 1))


def _spec(desc, name=None, **kw):
    name = name or ("Navier_Stokes" if desc.k == 3 else "physics_equation")
    ins = ("t", "x", "y") if desc.k == 3 else ("x", "y")
    outs = {"Navier_Stokes": NS_OUT, "physics_equation": PE_OUT}.get(name, ("h", "U", "V"))
    return ResidualSpec.from_names(name, ins, desc.grad_cols, outs, **kw)


def _call(desc, spec, nu=0.1):
    lib = _lib.load()
    rc = lib.pinn_residual2_loss_grad(C.byref(desc.c_struct()), C.byref(spec.c_struct()), C.c_float(nu), _P, _P, _P, 64, _P, _P, _P,
                                      _P, 1 << 40, None)
    return rc, lib.pinn_last_error().decode()


def _query(desc, spec):
    lib = _lib.load()
    need = C.c_int64(-1)
    rc = lib.pinn_query_residual2_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), 64, C.byref(need))
    return rc, lib.pinn_last_error().decode(), need.value


def _jet2_query(desc):
    lib = _lib.load()
    need = C.c_int64(-1)
    rc = lib.pinn_query_jet2_workspace(C.byref(desc.c_struct()), 64, C.byref(need))
    return rc, lib.pinn_last_error().decode()


@pytest.mark.parametrize("nu", [-1e-3, float("nan"), float("inf"), -float("inf")])
def test_call_refuses_a_negative_or_non_finite_nu(nu):
    rc, msg = _call(NS, _spec(NS), nu)
    assert rc == ERR_INVALID and "nu" in msg


def test_k_must_equal_the_residuals_directions():
    d3 = NetDesc(3, 6, 3, 20, (0, 1, 2))
    s = ResidualSpec.from_names("physics_equation", ("x", "y", "t"), d3.grad_cols, PE_OUT)
    d2 = NetDesc(3, 4, 3, 20, (0, 1))
    s2 = ResidualSpec("Navier_Stokes", (0, 1, 2, 3), (0, 1, 1))
    for desc, spec in ((d3, s), (d2, s2)):
        rc, msg = _call(desc, spec)
        assert rc == ERR_UNSUPPORTED and "directions" in msg
        assert _query(desc, spec)[:2] == (rc, msg)


@pytest.mark.parametrize("name", ["continuity_ftemp", "continuity_only"])
def test_continuity_residuals_are_refused(name):
    d = NetDesc(2, 3, 3, 20, (0, 1))
    spec = _spec(d, name)
    rc, msg = _call(d, spec)
    assert rc == ERR_UNSUPPORTED and "no second-order term" in msg
    assert _query(d, spec)[:2] == (rc, msg)
    with pytest.raises(PinnError, match="momentum"):
        _spec(d, name, nu=0.1)
    assert _spec(d, name, nu=0.0).nu == 0.0


FUSED_REFUSED = {
    "width 256": (NS.with_(width=256, n_hidden=3), "at most 64 wide"),
    "d_in 65": (NetDesc(65, 4, 2, 32, (0, 1, 2)), "at most 64 wide"),
    "dropout": (NS.with_(dropout_p=0.1), "dropout_p > 0"),
}


@pytest.mark.parametrize("case", sorted(FUSED_REFUSED))
@pytest.mark.parametrize("engine", [ENGINE_FUSED, ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH])
def test_fused_refuses_with_the_messages_of_forward_jet2(case, engine):
    desc, word = FUSED_REFUSED[case]
    desc = desc.with_(engine=engine)
    rc, msg = _call(desc, _spec(desc))
    assert rc == ERR_UNSUPPORTED and word in msg
    assert (rc, msg) == _jet2_query(desc) and _query(desc, _spec(desc))[:2] == (rc, msg)
    for e in (ENGINE_AUTO, ENGINE_GENERIC):          # served there
        d = desc.with_(engine=e)
        q = _query(d, _spec(d))
        assert q[0] == 0 and q[2] > 0, q


@pytest.mark.parametrize("case", ["WIDE", "bf16", "bf16 GENERIC"])
def test_wide_and_bf16_are_refused(case):
    desc = {"WIDE": NS.with_(width=128, engine=ENGINE_WIDE), "bf16": NS.with_(width=128, precision=PREC_BF16),
            "bf16 GENERIC": NS.with_(precision=PREC_BF16, engine=ENGINE_GENERIC)}[case]
    rc, msg = _call(desc, _spec(desc))
    assert rc == ERR_UNSUPPORTED and (rc, msg) == _jet2_query(desc) and _query(desc, _spec(desc))[:2] == (rc, msg)


def test_served_requests_pass_validation_and_answer_the_query():
    for desc in (NS, PE, PE.with_(activation=ACT_LEAKY_RELU), NS.with_(engine=ENGINE_GENERIC, dropout_p=0.2),
                 NS.with_(engine=ENGINE_FUSED)):
        for kw in ({}, {"corrected": True}) if desc.k == 2 else ({},):
            rc, msg, need = _query(desc, _spec(desc, **kw))
            assert rc == 0 and need > 0, msg
    # the workspace is the jet2 one plus the partial sums
    lib = _lib.load()
    j2 = C.c_int64()
    assert lib.pinn_query_jet2_workspace(C.byref(NS.c_struct()), 64, C.byref(j2)) == 0
    assert 0 < _query(NS, _spec(NS))[2] - j2.value <= 4096
    # nu == 0 is a valid request: with the fake pointers it gets past validation to the NULL-free argument check, and N = 0
    # is refused by nothing
    assert lib.pinn_residual2_loss_grad(C.byref(NS.c_struct()), C.byref(_spec(NS).c_struct()), C.c_float(0.0), None, None, None, 64,
                                        None, None, None, None, 0, None) == ERR_INVALID
    assert "NULL" in lib.pinn_last_error().decode()


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_spec_carries_nu_beside_the_c_struct():
    s = _spec(NS, nu=0.25)
    assert s.nu == 0.25 and _spec(NS).nu == 0.0 and ResidualSpec("Navier_Stokes", (0, 1, 2, 3), (0, 1, 2)).nu == 0.0
    assert C.sizeof(s.c_struct()) == C.sizeof(_spec(NS).c_struct()) and bytes(s.c_struct()) == bytes(_spec(NS).c_struct())
    assert _spec(PE, corrected=True, nu=0.5).corrected
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(PinnError, match="nu"):
            _spec(NS, nu=bad)
    for sym in ("pinn_residual2_point", "pinn_query_residual2_workspace", "pinn_residual2_loss_grad"):
        assert sym in _lib.exported_symbols()
    assert _lib.load().pinn_version() == _lib.ABI_VERSION == 4


def test_first_order_engine_methods_do_not_drop_nu():
    eng = Engine(NS, "cpu")
    s = _spec(NS, nu=0.1)
    t = torch.zeros(1)
    calls = {
        "residual_loss": lambda: eng.residual_loss(s, t, t),
        "residual_fields": lambda: eng.residual_fields(s, t, t),
        "fields_workspace": lambda: eng.fields_workspace(s, 16),
        "residual_loss_grad": lambda: eng.residual_loss_grad(s, t, t, t, t),
        "residual_mse_loss_grad": lambda: eng.residual_mse_loss_grad(s, t, t, (0,), t, t, t, t),
        "residual_mse_split_loss_grad": lambda: eng.residual_mse_split_loss_grad(s, t, t, (0,), t, t, t, 0, t),
        "loss_grad_adam_step": lambda: eng.loss_grad_adam_step(s, t, t, t, 0, t, t, t, 1, 1e-3),
    }
    for name, fn in calls.items():
        with pytest.raises(PinnError, match="nu = 0.1"):
            fn()


# ---- trainer and tester (after the plumbing checks of test_pe_corrected_cpu.py) -----------------------------------------
from tests.test_pe_corrected_cpu import _cfg, _pinn      # noqa: E402


def test_trainer_keyword_and_config_key():
    assert _pinn(_cfg(PE_OUT)).spec.nu == 0.0 and _pinn(_cfg(PE_OUT)).eddy_viscosity == 0.0
    tr = _pinn(_cfg(PE_OUT), eddy_viscosity=0.05)
    assert tr.eddy_viscosity == 0.05 and tr.spec.nu == 0.05 and not tr.spec.corrected
    tr = _pinn(_cfg(PE_OUT, eddy_viscosity=0.2, corrected_radiation_stress=True))
    assert tr.spec.nu == pytest.approx(0.2) and tr.spec.corrected and tr.spec.c_struct().flags == 1
    assert _pinn(_cfg(PE_OUT, eddy_viscosity=0.2), eddy_viscosity=0.3).spec.nu == pytest.approx(0.3)      # the keyword wins
    with pytest.raises(PinnError, match="momentum"):
        _pinn(_cfg(("U", "V", "h")), eddy_viscosity=0.1, residual="continuity_ftemp")
    with pytest.raises(PinnError, match="momentum"):
        _pinn(_cfg(("U", "V", "h"), eddy_viscosity=0.1))
    with pytest.raises(PinnError, match="nu"):
        _pinn(_cfg(PE_OUT), eddy_viscosity=-0.1)


def test_hip_evaluator_routes_nu_to_the_second_order_entry():
    """Which Engine method each request reaches, on recording stand-ins: no device."""
    from pinn_depthestimation_amd.trainer import HipEvaluator

    class Rec:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def f(*a, **kw):
                self.calls.append(name)
                return (None, "F") if kw.get("fields") else False
            return f

    for nu in (0.0, 0.1):
        ev = HipEvaluator.__new__(HipEvaluator)
        ev.eng, ev.eng_drop, ev.training, ev.fid_cols, ev.merge_sets = Rec(), None, True, [0], True
        ev._cat, ev._cat_src = None, (None, None)
        ev.spec = _spec(PE, nu=nu)
        X, Xf, z = torch.zeros(8, 2), torch.zeros(4, 2), torch.zeros(3)
        ev(z, Xf, z, z, X, z, z, z, z)
        folded = ev.adam_iteration(z, Xf, z, z, X, z, z, z, z, z, z, 1, 1e-3)
        ev.residual_fields(z, X)
        if nu:
            assert ev.eng.calls == ["mse_loss_grad", "residual2_loss_grad", "residual2_loss_grad"] and folded is False
        else:
            assert ev.eng.calls == ["residual_mse_split_loss_grad", "loss_grad_adam_step", "residual_fields"]


def test_tester_keyword():
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.inference import Tester
    cfg = _cfg(PE_OUT)
    t = Tester(DNN([2, 10, 10, 6], 0.0, "xavier"), cfg, device="cpu", eddy_viscosity=0.05)
    assert t.eddy_viscosity == 0.05 and Tester(DNN([2, 10, 10, 6], 0.0, "xavier"), cfg, device="cpu").eddy_viscosity == 0.0
    with pytest.raises(PinnError, match="eddy_viscosity"):
        Tester(DNN([2, 10, 10, 6], 0.0, "xavier"), cfg, device="cpu", eddy_viscosity=-1.0)
    with pytest.raises(PinnError, match="momentum"):
        Tester(DNN([2, 10, 10, 3], 0.0, "xavier"), _cfg(("U", "V", "h")), device="cpu", residual="continuity_ftemp", eddy_viscosity=0.1)


def test_physics_formula_route_matches_the_reference_formula_on_plain_tensors():
    """physics.Navier_Stokes / physics_equation(nu=...) on tensors that come from no DNN.forward call: nested compute_gradient."""
    from pinn_depthestimation_amd import physics
    for case, (name, corrected) in CASES.items():
        nr, nd, dx, dy = SHAPE[name]
        V, LAP = _jets(name, 50, 31)
        V64 = torch.tensor(V, dtype=torch.float64).reshape(50, 1 + nd, nr)
        ins = [torch.zeros(50, 1, dtype=torch.float64, requires_grad=True) for _ in range(nd)]
        outs = []
        for r in range(nr):
            a = V64[:, 0, r:r + 1] + sum(V64[:, 1 + d, r:r + 1] * ins[d] for d in range(nd))
            if r in MOM[name]:
                a = a + 0.25 * float(LAP[0, 0]) * (ins[dx] ** 2 + ins[dy] ** 2)
            outs.append(a)
        want = sum(torch.mean(f ** 2) for f in formula(name, corrected, 0.3, ins, outs))
        kw = {"corrected": True} if corrected else {}
        got = getattr(physics, name)(*ins, *outs, nu=0.3, **kw)
        assert float(got.detach()) == pytest.approx(float(want.detach()), rel=1e-13)
        assert float(got.detach()) != pytest.approx(float(getattr(physics, name)(*ins, *outs, **kw).detach()), rel=1e-6)

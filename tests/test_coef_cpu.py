"""Runtime closure coefficients (gamma_b of Navier_Stokes, Cd of physics_equation), everything that needs no GPU: the host
evaluation pinn_residual_coef_point — the very functions the kernels call — against torch autograd in float64 over the
Python formula (tests/coef_util.formula), the defaults against the existing host entry, the misreadings the GPU test's
bounds must see, the refusals of pinn_residual_coef_loss_grad and its workspace query (made before any device work), and the
plumbing through ResidualSpec, physics, the config and the trainer."""
import ctypes as C

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import NetDesc, ResidualSpec, _lib
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, ERR_INVALID, ERR_UNSUPPORTED, PREC_BF16,
                                           PinnError)
from tests import coef_util as U
from tests.test_pe_corrected_cpu import _jets as pe_jets
from tests.test_residual2_cpu import _ns_jets, _point as res2_point

FP = C.POINTER(C.c_float)
SCALE = (0.7, 1.3, 0.9)
RID = {"Navier_Stokes": _lib.RES_NAVIER_STOKES, "physics_equation": _lib.RES_PHYSICS_EQUATION}
SHAPE = {"Navier_Stokes": (4, 3), "physics_equation": (6, 2)}     # roles, directions


def _jets(name, n, seed):
    return _ns_jets(n, seed) if name == "Navier_Stokes" else pe_jets(n, seed)


def _point(rid, v, coef, scale=SCALE, want_g=True, want_gc=True, fill=0.0):
    """One call: -> (rc, fields (3,), g (len(v),), gcoef (1,))."""
    lib = _lib.load()
    v = np.ascontiguousarray(v, dtype=np.float32)
    cf = None if coef is None else np.ascontiguousarray([coef], dtype=np.float32)
    f = np.zeros(3, np.float32)
    g = np.full(len(v), fill, np.float32)
    gc = np.full(1, fill, np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    rc = lib.pinn_residual_coef_point(rid, v.ctypes.data_as(FP), None if cf is None else cf.ctypes.data_as(FP),
                                      None if sc is None else sc.ctypes.data_as(FP), f.ctypes.data_as(FP),
                                      g.ctypes.data_as(FP) if want_g else None, gc.ctypes.data_as(FP) if want_gc else None)
    return rc, f, g, gc


def _host_all(name, coef, V):
    F, Gv, GC = np.zeros((len(V), 3), np.float32), np.zeros(V.shape, np.float32), np.zeros(len(V), np.float32)
    for i in range(len(V)):
        rc, F[i], Gv[i], gc = _point(RID[name], V[i], coef)
        assert rc == 0
        GC[i] = gc[0]
    return F, Gv, GC


def _autograd_reference(name, coef, V, scale=SCALE):
    """fp64 fields (n, 3), adjoint of the jet (n, .) and per-point coefficient gradient (n,) of sum_t scale[t] field_t^2: each
    role is the linear function of the inputs whose value and gradient at the origin are the jet's."""
    nr, nd = SHAPE[name]
    n = len(V)
    V64 = torch.tensor(V, dtype=torch.float64).reshape(n, 1 + nd, nr).requires_grad_(True)
    cvec = torch.full((n, 1), coef, dtype=torch.float64, requires_grad=True)
    ins = [torch.zeros(n, 1, dtype=torch.float64, requires_grad=True) for _ in range(nd)]
    outs = []
    for r in range(nr):
        a = V64[:, 0, r:r + 1]
        for d in range(nd):
            a = a + V64[:, 1 + d, r:r + 1] * ins[d]
        outs.append(a)
    f = torch.cat(U.formula(name, cvec, ins, outs), dim=1)
    obj = (f ** 2 * torch.tensor(scale, dtype=torch.float64)).sum()
    g, gc = torch.autograd.grad(obj, (V64, cvec))
    return f.detach().numpy(), g.reshape(n, -1).numpy(), gc.reshape(-1).numpy()


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


# ---- 1. the host point evaluator against fp64 autograd --------------------------------------------------------------------
@pytest.mark.parametrize("name,coef", [("Navier_Stokes", 0.78), ("Navier_Stokes", 0.4), ("physics_equation", 0.002),
                                       ("physics_equation", 0.5)])
def test_point_matches_fp64_autograd(name, coef):
    V = _jets(name, 4000, 21)
    F, Gv, GC = _host_all(name, coef, V)
    Fr, Gr, GCr = _autograd_reference(name, coef, V)
    ef, eg, ec = _rel_l2(F, Fr), _rel_l2(Gv, Gr), _rel_l2(GC, GCr)
    print(f"{name} {U.COEF_NAME[name]}={coef}: fields rel_l2 {ef:.2e}, adjoint rel_l2 {eg:.2e}, gcoef rel_l2 {ec:.2e}")
    assert ef < 2e-6 and eg < 2e-5 and ec < 2e-5


# ---- 2. the defaults against the existing host entry ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Navier_Stokes", "physics_equation"])
def test_default_coefficient_is_the_existing_host_entry_to_rounding(name):
    """Not bitwise: rho Cd and 3/16 g gamma_b^2 are formed in fp32 at run time here, in double at compile time there."""
    V = _jets(name, 1000, 22)
    F, Gv, _ = _host_all(name, U.DEFAULTS[name], V)
    F0, G0 = np.zeros_like(F), np.zeros_like(Gv)
    for i, v in enumerate(V):
        rc, F0[i], G0[i], gl = res2_point(name, False, 0.0, v, np.zeros(2, np.float32), scale=SCALE)
        assert rc == 0 and not gl.any()
    ef, eg = _rel_l2(F, F0.astype(np.float64)), _rel_l2(Gv, G0.astype(np.float64))
    print(f"{name}: default coefficient against pinn_residual2_point(nu = 0): fields {ef:.2e}, adjoint {eg:.2e}")
    assert ef < 2e-6 and eg < 2e-6


def test_counts_and_defaults():
    lib = _lib.load()
    n = C.c_int32(-1)
    for rid, flags, want in ((1, 0, 1), (2, 0, 1), (3, 0, 0), (4, 0, 0), (2, 1, 0), (1, 1, 1)):
        assert lib.pinn_residual_coef_count(rid, flags, C.byref(n)) == 0 and n.value == want, (rid, flags)
    assert lib.pinn_residual_coef_count(9, 0, C.byref(n)) == ERR_INVALID
    assert lib.pinn_residual_coef_count(1, 0, None) == ERR_INVALID
    v = C.c_float()
    assert lib.pinn_residual_coef_default(1, 0, C.byref(v)) == 0 and v.value == np.float32(0.78)
    assert lib.pinn_residual_coef_default(2, 0, C.byref(v)) == 0 and v.value == np.float32(0.002)
    assert lib.pinn_residual_coef_default(1, 1, C.byref(v)) == ERR_INVALID
    assert lib.pinn_residual_coef_default(1, 0, None) == ERR_INVALID
    for rid in (3, 4):
        assert lib.pinn_residual_coef_default(rid, 0, C.byref(v)) == ERR_UNSUPPORTED
        assert "no coefficient" in lib.pinn_last_error().decode()
    ns = ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), (0, 1, 2), ("h", "z", "u", "v"))
    pe = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ("h", "U", "V", "eta_mean", "Hrms", "k"))
    pec = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ("h", "U", "V", "eta_mean", "Hrms", "k"), corrected=True)
    cf = ResidualSpec.from_names("continuity_ftemp", ("x", "y"), (0, 1), ("h", "U", "V"))
    assert (ns.n_coefs, ns.coef_names, ns.coef_defaults) == (1, ("gamma_b",), (float(np.float32(0.78)),))
    assert (pe.n_coefs, pe.coef_names, pe.coef_defaults) == (1, ("Cd",), (float(np.float32(0.002)),))
    assert (pec.n_coefs, pec.coef_names, pec.coef_defaults) == (0, (), ())
    assert (cf.n_coefs, cf.coef_names, cf.coef_defaults) == (0, (), ())
    assert _lib.PINN_MAX_COEFS == 4


def test_point_null_arguments_and_refusals():
    lib = _lib.load()
    V = _jets("Navier_Stokes", 1, 23)
    _, f0, g0, gc0 = _point(1, V[0], 0.6)
    for kw in (dict(scale=None), dict(want_g=False), dict(want_gc=False)):      # any of the three NULL: fields only
        rc, f1, g1, gc1 = _point(1, V[0], 0.6, fill=7.0, **kw)
        assert rc == 0 and np.array_equal(f0, f1) and np.all(g1 == 7.0) and np.all(gc1 == 7.0), kw
    assert _point(1, V[0], None)[0] == ERR_INVALID and "NULL" in lib.pinn_last_error().decode()
    for rid in (3, 4):
        assert _point(rid, V[0], 0.6)[0] == ERR_UNSUPPORTED and "no coefficient" in lib.pinn_last_error().decode()
    assert _point(7, V[0], 0.6)[0] == ERR_INVALID


# ---- 3. misreadings: the GPU test's bounds see them -----------------------------------------------------------------------
def _gpu_cases():
    out = [(s, N, c) for s in U.TILE_SHAPES for c in U.COEFS[U.SHAPES[s][0]] for N in U.POINTS]
    return out + [(U.LARGE[0], U.LARGE[2], U.LARGE[1])]


def test_gpu_bounds_see_an_ignored_coefficient():
    """The coefficient ignored (the default used): at every non-default case, sums, parameter gradient or coefficient
    gradient of the default's evaluation miss the bounds test_coef_gpu holds the kernels to."""
    n = 0
    for shape, N, coef in _gpu_cases():
        res = U.SHAPES[shape][0]
        if coef == U.DEFAULTS[res]:
            continue
        r64, r32 = U.reference(shape, N, coef)
        wrong, _ = U.reference(shape, N, U.DEFAULTS[res])
        ratios = (U.sums_ratio(wrong.sums, r64, r32), U.grad_ratio_unasserted(wrong.grad, r64, r32, list(U.SHAPES[shape][1])),
                  U.coef_grad_ratio(wrong.gc, r64, r32))
        assert max(ratios) > 1.0, (shape, N, coef, ratios)
        n += 1
    assert n == len(U.TILE_SHAPES) * len(U.POINTS) + 1


def test_gpu_bounds_see_a_dropped_factor():
    """gcoef without the 3/8 g gamma_b factor (Navier_Stokes): every case misses the coefficient-gradient bound."""
    for shape, N, coef in _gpu_cases():
        if U.SHAPES[shape][0] != "Navier_Stokes":
            continue
        r64, r32 = U.reference(shape, N, coef)
        wrong = r64.gc / (3.0 / 8.0 * U.G * coef)
        assert U.coef_grad_ratio(wrong, r64, r32) > 1.0, (shape, N, coef)


def test_gpu_bounds_see_rx_and_ry_exchanged():
    """gcoef with rx and ry exchanged: sum_n (ry df_x/dc + rx df_y/dc).  One point, or a set on which the two happen to agree,
    could hide it; the cases from 15 points on do not."""
    seen = 0
    for shape, N, coef in _gpu_cases():
        r64, r32 = U.reference(shape, N, coef)
        right = float((r64.rx * r64.dfx + r64.ry * r64.dfy).sum())
        assert abs(right - r64.gc) <= 1e-9 * r64.A                       # (the decomposition is the gradient)
        wrong = float((r64.ry * r64.dfx + r64.rx * r64.dfy).sum())
        if N >= 15:
            assert U.coef_grad_ratio(wrong, r64, r32) > 1.0, (shape, N, coef)
            seen += 1
    assert seen > 0


# ---- 4. host logic that needs no device ------------------------------------------------------------------------------------
NS_SPEC = ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), (0, 1, 2), ("h", "z", "u", "v"))
PE_SPEC = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ("h", "U", "V", "eta_mean", "Hrms", "k"))


def _query(desc, spec, N=100):
    lib = _lib.load()
    b = C.c_int64(-1)
    rc = lib.pinn_query_residual_coef_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), N, C.byref(b))
    return rc, b.value, lib.pinn_last_error().decode()


def _call(desc, spec, coef=None):
    """The loss entry with NULL buffers: a refusal by the rules comes first, a served request ends at 'NULL pointer'."""
    lib = _lib.load()
    rc = lib.pinn_residual_coef_loss_grad(C.byref(desc.c_struct()), C.byref(spec.c_struct()), coef, None, None, None, 100, None,
                                          None, None, None, 0, None)
    return rc, lib.pinn_last_error().decode()


REFUSED = [
    # (what, descriptor, spec, word in the message)
    ("k != directions", NetDesc(3, 4, 2, 10, (0, 1)), ResidualSpec("Navier_Stokes", (0, 1, 2, 3), (0, 1, 1)), "directions"),
    ("corrected", NetDesc(2, 6, 2, 10, (0, 1)), ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ("h", "U", "V", "eta_mean", "Hrms", "k"), corrected=True), "corrected"),
    ("continuity_ftemp", NetDesc(2, 3, 2, 10, (0, 1)), ResidualSpec.from_names("continuity_ftemp", ("x", "y"), (0, 1), ("h", "U", "V")), "no coefficient"),
    ("continuity_only", NetDesc(2, 3, 2, 10, (0, 1)), ResidualSpec.from_names("continuity_only", ("x", "y"), (0, 1), ("h", "U", "V")), "no coefficient"),
    ("fused, LeakyReLU", NetDesc(3, 4, 2, 10, (0, 1, 2), activation=ACT_LEAKY_RELU, engine=ENGINE_FUSED), NS_SPEC, "LeakyReLU"),
    ("fused tile, width 100", NetDesc(2, 6, 2, 100, (0, 1), engine=ENGINE_FUSED_TILE), PE_SPEC, "width"),
    ("fused, d_out 17", NetDesc(2, 17, 2, 10, (0, 1), engine=ENGINE_FUSED), PE_SPEC, "d_out"),
    ("fused, dropout", NetDesc(2, 6, 2, 10, (0, 1), engine=ENGINE_FUSED, dropout_p=0.1), PE_SPEC, "dropout"),
    ("fused coop", NetDesc(3, 4, 2, 64, (0, 1, 2), engine=ENGINE_FUSED_COOP), NS_SPEC, "FUSED_COOP"),
    ("fused batch", NetDesc(2, 6, 2, 10, (0, 1), engine=ENGINE_FUSED_BATCH), PE_SPEC, "FUSED_BATCH"),
    ("wide", NetDesc(2, 6, 2, 128, (0, 1), engine=ENGINE_WIDE), PE_SPEC, "wide"),
    ("bf16", NetDesc(2, 6, 2, 128, (0, 1), precision=PREC_BF16), PE_SPEC, "bf16"),
]
SERVED = [
    ("generic, any shape", NetDesc(2, 20, 3, 100, (0, 1), activation=ACT_LEAKY_RELU, engine=ENGINE_GENERIC, dropout_p=0.2), PE_SPEC),
    ("fused", NetDesc(3, 4, 2, 64, (0, 1, 2), engine=ENGINE_FUSED), NS_SPEC),
    ("fused tile", NetDesc(2, 6, 2, 10, (0, 1), engine=ENGINE_FUSED_TILE), PE_SPEC),
    ("auto, tile shape", NetDesc(2, 6, 2, 10, (0, 1), engine=ENGINE_AUTO), PE_SPEC),
    ("auto, width 100 -> generic", NetDesc(2, 6, 2, 100, (0, 1), engine=ENGINE_AUTO), PE_SPEC),
    ("auto, LeakyReLU -> generic", NetDesc(3, 4, 2, 10, (0, 1, 2), activation=ACT_LEAKY_RELU), NS_SPEC),
    ("auto, dropout -> generic", NetDesc(3, 4, 2, 64, (0, 1, 2), dropout_p=0.3), NS_SPEC),
]


@pytest.mark.parametrize("what,desc,spec,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusal_table_without_a_device(what, desc, spec, word):
    one = (C.c_float * 1)(0.5)
    rc, msg = _call(desc, spec, C.cast(one, C.c_void_p))
    assert rc == ERR_UNSUPPORTED and word in msg, (what, rc, msg)
    rc, _, msg = _query(desc, spec)
    assert rc == ERR_UNSUPPORTED and word in msg, (what, rc, msg)


@pytest.mark.parametrize("what,desc,spec", SERVED, ids=[r[0] for r in SERVED])
def test_served_rows_pass_the_rules_without_a_device(what, desc, spec):
    rc, nbytes, msg = _query(desc, spec)
    assert rc == 0 and nbytes > 0, (what, rc, msg)
    one = (C.c_float * 1)(0.5)
    rc, msg = _call(desc, spec, C.cast(one, C.c_void_p))
    assert rc == ERR_INVALID and "NULL" in msg, (what, rc, msg)


def test_auto_moves_between_engines_and_the_query_follows():
    """AUTO's workspace is the tile kernel's where FUSED is served and the generic engine's elsewhere."""
    for desc, same_as in ((NetDesc(2, 6, 2, 10, (0, 1)), ENGINE_FUSED_TILE), (NetDesc(2, 6, 2, 100, (0, 1)), ENGINE_GENERIC)):
        assert _query(desc, PE_SPEC, 5000)[1] == _query(desc.with_(engine=same_as), PE_SPEC, 5000)[1]
    assert _query(NetDesc(2, 6, 2, 10, (0, 1)), PE_SPEC, 5000)[1] != _query(NetDesc(2, 6, 2, 10, (0, 1), engine=ENGINE_GENERIC), PE_SPEC, 5000)[1]


def test_null_arguments():
    lib = _lib.load()
    desc = NetDesc(2, 6, 2, 10, (0, 1))
    rc, msg = _call(desc, PE_SPEC, None)                                  # coef == NULL
    assert rc == ERR_INVALID and "NULL" in msg
    assert lib.pinn_query_residual_coef_workspace(C.byref(desc.c_struct()), C.byref(PE_SPEC.c_struct()), 10, None) == ERR_INVALID
    assert lib.pinn_query_residual_coef_workspace(C.byref(desc.c_struct()), None, 10, C.byref(C.c_int64())) == ERR_INVALID
    assert lib.pinn_query_residual_coef_workspace(None, C.byref(PE_SPEC.c_struct()), 10, C.byref(C.c_int64())) == ERR_INVALID
    # coef_grad without grad_flat: the coefficient gradient comes out of the gradient pass
    one = (C.c_float * 4)(0.5, 0, 0, 0)
    p = C.cast(one, C.c_void_p)
    rc = lib.pinn_residual_coef_loss_grad(C.byref(desc.c_struct()), C.byref(PE_SPEC.c_struct()), p, None, p, p, 1, p, None, p, None, 0, None)
    assert rc == ERR_INVALID and "coef_grad" in lib.pinn_last_error().decode()


def test_formula_route_takes_the_coefficient_and_differentiates_it():
    """physics.Navier_Stokes(gamma_b=...) / physics_equation(Cd=...) on plain tensors (no engine behind them: the formula)."""
    from pinn_depthestimation_amd import physics
    g = torch.Generator().manual_seed(3)
    x, y, t = (torch.rand(50, 1, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3))
    h, U_, V_, eta, Hrms, k = 2 + 0.1 * x * y, 0.3 * x - 0.2 * y, 0.1 * x * x + y, 0.2 * x + 0.1 * y, 0.5 + 0 * x, 1 + 0 * x
    cd = torch.tensor(0.05, dtype=torch.float64, requires_grad=True)
    loss = physics.physics_equation(x, y, h, U_, V_, eta, Hrms, k, Cd=cd)
    (gcd,) = torch.autograd.grad(loss, cd)
    f = torch.cat(U.formula("physics_equation", cd, (x, y), (h, U_, V_, eta, Hrms, k)), 1)
    want = (f ** 2).mean(0).sum()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach())) and float(gcd) != 0.0
    assert abs(float(gcd) - float(torch.autograd.grad(want, cd)[0])) <= 1e-12 * abs(float(gcd))
    assert torch.equal(physics.physics_equation(x, y, h, U_, V_, eta, Hrms, k, Cd=0.002), physics.physics_equation(x, y, h, U_, V_, eta, Hrms, k))
    z, u, v = 0.2 + 0.1 * t * x + 0.05 * y, 0.3 * x - 0.2 * t + 0.1 * y, 0.1 * y + t + 0.2 * x
    gb = torch.tensor(0.6, dtype=torch.float64, requires_grad=True)
    loss = physics.Navier_Stokes(t, x, y, h, z, u, v, gamma_b=gb)
    f = torch.cat(U.formula("Navier_Stokes", gb, (t, x, y), (h, z, u, v)), 1)
    want = (f ** 2).mean(0).sum()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    assert float(torch.autograd.grad(loss, gb)[0]) != 0.0
    assert torch.equal(physics.Navier_Stokes(t, x, y, h, z, u, v, gamma_b=0.78), physics.Navier_Stokes(t, x, y, h, z, u, v))


# ---- the trainer: config parsing and refusals, all before anything touches a device -----------------------------------------
def _cfg(**loss):
    return {
        "layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0, "init_type": "xavier"},
        "adam_optimizer": {"max_it": 20, "learning_rate": 1e-3, "scheduler_step_size": 7, "scheduler_gamma": 0.8},
        "lbfgs_optimizer": {"max_it": 0, "learning_rate": 1, "max_evaluation": 100, "history_size": 10,
                            "tolerance_grad": 1e-5, "tolerance_change": 1e-7, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1, **{f"weight_{k}_loss": 1 for k in ("h", "U", "V", "eta_mean", "Hrms", "k")}, **loss},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": ["h", "U", "V", "eta_mean", "Hrms", "k"], "training_points": 12},
        "data_residual": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}},
                          "outputs": ["h", "U", "V", "eta_mean", "Hrms", "k"]},
    }


def test_coefficient_refusal_rules():
    from pinn_depthestimation_amd.trainer import coefficient_refusal as R, device_lbfgs_refusal as D
    assert R("physics_equation", {}, ()) is None
    assert R("physics_equation", {"Cd": 0.01}, ("Cd",)) is None
    assert R("Navier_Stokes", {}, ("gamma_b",)) is None
    assert "gamma_b" in R("physics_equation", {"gamma_b": 0.5}, ())
    assert "Cd" in R("Navier_Stokes", {}, ("Cd",))
    assert "no coefficient" in R("continuity_ftemp", {"Cd": 0.01}, ())
    assert "corrected" in R("physics_equation", {"Cd": 0.01}, (), corrected=True)
    assert "eddy_viscosity" in R("physics_equation", {"Cd": 0.01}, (), eddy_viscosity=0.1)
    assert "data parallelism" in R("physics_equation", {"Cd": 0.01}, (), reducer_active=True)
    assert "rad" in R("physics_equation", {"Cd": 0.01}, (), resample="rad")
    assert "evaluator" in R("physics_equation", {"Cd": 0.01}, (), custom_evaluator=True)
    assert D(False, None, 0.0, False, "strong_wolfe") is None
    assert "coefficients" in D(False, None, 0.0, False, "strong_wolfe", 0.0, True)


class _ActiveReducer:
    active, rank, world = True, 0, 2


@pytest.mark.parametrize("kw,cfg_loss,word", [
    (dict(coefficients={"Cd": 0.01}, lbfgs_impl="device"), {}, "device"),
    (dict(trainable_coefficients=("Cd",), reducer=_ActiveReducer()), {}, "data parallelism"),
    (dict(coefficients={"Cd": 0.01}, eddy_viscosity=0.1), {}, "eddy_viscosity"),
    (dict(coefficients={"Cd": 0.01}, corrected=True), {}, "corrected"),
    (dict(coefficients={"Cd": 0.01}, resample="rad", residual_batch=10), {}, "rad"),
    (dict(coefficients={"gamma_b": 0.5}), {}, "gamma_b"),
    (dict(trainable_coefficients=("Cf",)), {}, "Cf"),
    (dict(), {"coefficients": {"Cd": 0.01}, "corrected_radiation_stress": True}, "corrected"),      # the config keys
    (dict(), {"trainable_coefficients": ["gamma_b"]}, "gamma_b"),
    (dict(lbfgs_impl="device"), {"coefficients": {"Cd": 0.01}}, "device"),
])
def test_trainer_refuses_before_touching_a_device(kw, cfg_loss, word):
    from pinn_depthestimation_amd.trainer import PINN
    X = np.zeros((4, 2), np.float32)
    with pytest.raises(PinnError, match=word):
        PINN(X, np.zeros((4, 6), np.float32), X, _cfg(**cfg_loss), **kw)


def test_ensemble_refuses_coefficients():
    from pinn_depthestimation_amd.ensemble import EnsemblePINN
    X = np.zeros((4, 2), np.float32)
    with pytest.raises(PinnError, match="coefficients"):
        EnsemblePINN(X, np.zeros((4, 6), np.float32), X, _cfg(), 2, coefficients={"Cd": 0.01})
    with pytest.raises(PinnError, match="coefficients"):
        EnsemblePINN(X, np.zeros((4, 6), np.float32), X, _cfg(trainable_coefficients=["Cd"]), 2)

"""The wave closure of the corrected physics_equation (pinn_residual_spec.flags bits 0 and 1: the dispersion relation and the
wave-energy balance as a fourth and a fifth term), everything that needs no GPU: the host evaluation pinn_pe_wave_point —
the very functions the kernels call — against torch autograd in float64 over the Python formula, terms 0..2 against
pinn_pe_corrected_point bit for bit, the plumbing of the flag, the C-ABI's validation and refusals (made before any device
work) over descriptor x engine, and the trainer's options.

Bars: the corrected residual's (test_pe_corrected_cpu.py) — fields rel_l2 2e-6, adjoint rel_l2 2e-5."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import NetDesc, ResidualSpec, _lib, physics
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ACT_SIN_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE,
                                           PREC_BF16, PinnError)
from tests.pe_corrected_util import ROLES
from tests.pe_wave_util import wave_fields, wave_loss

PE_IN = ("x", "y")
FP = C.POINTER(C.c_float)


def _spec(desc, omega=2.5, gamma=0.42, inputs=PE_IN):
    return ResidualSpec.from_names("physics_equation", inputs, desc.grad_cols, ROLES, corrected=True, wave_omega=omega, wave_gamma=gamma)


# ---- pinn_pe_wave_point against fp64 autograd over the formula -----------------------------------------------------------
def _point(v, omega, gamma, scale=None, want_g=True):
    """One call: v (18,) float32 -> (fields (5,), g (18,))."""
    lib = _lib.load()
    v = np.ascontiguousarray(v, dtype=np.float32)
    f, g = np.zeros(5, dtype=np.float32), np.zeros(18, dtype=np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    rc = lib.pinn_pe_wave_point(v.ctypes.data_as(FP), float(omega), float(gamma), None if sc is None else sc.ctypes.data_as(FP),
                                f.ctypes.data_as(FP), g.ctypes.data_as(FP) if want_g else None)
    assert rc == 0, lib.pinn_last_error()
    return f, g


def _corrected_point(v, scale):
    lib = _lib.load()
    v = np.ascontiguousarray(v, dtype=np.float32)
    f, g = np.zeros(3, dtype=np.float32), np.zeros(18, dtype=np.float32)
    sc = np.ascontiguousarray(scale, dtype=np.float32)
    assert lib.pinn_pe_corrected_point(v.ctypes.data_as(FP), sc.ctypes.data_as(FP), f.ctypes.data_as(FP), g.ctypes.data_as(FP)) == 0
    return f, g


def _autograd_reference(V, W, scale):
    """V (n, 18) float32 jets, W (n, 2) float32 (omega, gamma) -> fp64 fields (n, 5) and adjoint (n, 18) of
    sum_t scale[t] field_t^2, by torch autograd over the Python formula: each role is the affine function of (x, y) whose
    value and gradient at the point are the jet's."""
    V64 = torch.tensor(V, dtype=torch.float64).reshape(-1, 3, 6).requires_grad_(True)
    W64 = torch.tensor(W, dtype=torch.float64)
    n = V64.shape[0]
    x = torch.zeros(n, 1, dtype=torch.float64, requires_grad=True)
    y = torch.zeros(n, 1, dtype=torch.float64, requires_grad=True)
    outs = [V64[:, 0, r:r + 1] + V64[:, 1, r:r + 1] * x + V64[:, 2, r:r + 1] * y for r in range(6)]
    f = torch.cat(wave_fields(x, y, *outs, omega=W64[:, 0:1], gamma=W64[:, 1:2]), dim=1)
    obj = (f ** 2 * torch.tensor(scale, dtype=torch.float64)).sum()
    (g,) = torch.autograd.grad(obj, V64)
    return f.detach().numpy(), g.reshape(n, 18).numpy()


def _jets(n, seed, kh=None):
    """Random jets in the operating range the closure is meant for: h in [0.5, 6], Hrms in [0.1, 1.5], k in [0.05, 1.5],
    omega in [0.5, 3], gamma in [0.3, 0.8] (U, V, eta and the gradients as test_pe_corrected_cpu.py); with `kh` (n,) the
    wave number is set so that k h takes those values."""
    r = np.random.default_rng(seed)
    V = np.zeros((n, 3, 6))
    V[:, 0, 0] = r.uniform(0.5, 6.0, n)            # h
    V[:, 0, 1:3] = r.uniform(-0.5, 0.5, (n, 2))    # U, V
    V[:, 0, 3] = r.uniform(0.1, 0.3, n)            # eta
    V[:, 0, 4] = r.uniform(0.1, 1.5, n)            # Hrms
    V[:, 0, 5] = r.uniform(0.05, 1.5, n) if kh is None else kh / V[:, 0, 0]
    V[:, 1:, :] = r.uniform(-0.3, 0.3, (n, 2, 6))
    W = np.stack([r.uniform(0.5, 3.0, n), r.uniform(0.3, 0.8, n)], axis=1)
    return V.reshape(n, 18).astype(np.float32), W.astype(np.float32)


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


def _host_all(V, W, scale):
    F, G = np.zeros((len(V), 5), np.float32), np.zeros((len(V), 18), np.float32)
    for i, (v, w) in enumerate(zip(V, W)):
        F[i], G[i] = _point(v, w[0], w[1], scale)
    return F, G


SCALE = (0.7, 1.3, 0.9, 1.1, 0.8)
ONE_HOT = [tuple(1.0 if t == j else 0.0 for t in range(5)) for j in range(5)]


def _hold(tag, V, W):
    F, G = _host_all(V, W, SCALE)
    Fr, Gr = _autograd_reference(V, W, SCALE)
    ef, eg = _rel_l2(F, Fr), _rel_l2(G, Gr)
    per_field = [_rel_l2(F[:, t], Fr[:, t]) for t in range(5)]
    print(f"{tag}: fields rel_l2 {ef:.2e} (per field {[f'{e:.1e}' for e in per_field]}), adjoint rel_l2 {eg:.2e}")
    assert ef < 2e-6 and eg < 2e-5
    assert max(per_field) < 2e-6                      # each field by itself too: f_d is O(1), f_E small beside fx, fy
    for j, hot in enumerate(ONE_HOT):                 # each term alone
        _, Gj = _host_all(V, W, hot)
        _, Gjr = _autograd_reference(V, W, hot)
        e = _rel_l2(Gj, Gjr)
        print(f"{tag}: term {j} alone, adjoint rel_l2 {e:.2e}")
        assert e < 2e-5, j
    return F, G, Fr, Gr


def test_point_matches_fp64_autograd_in_the_operating_range():
    V, W = _jets(4000, 21)
    _hold("operating range", V, W)


def test_point_matches_fp64_autograd_for_kh_from_1e_minus_3_to_40():
    r = np.random.default_rng(22)
    kh = np.exp(r.uniform(np.log(1e-3), np.log(40.0), 4000))
    V, W = _jets(4000, 23, kh)
    F, G, Fr, Gr = _hold("kh in [1e-3, 40]", V, W)
    # ... and around the series / closed-form switch at kh = 1/4 (no jump there)
    near = np.abs(kh - 0.25) < 0.1
    assert near.sum() > 50
    assert _rel_l2(F[near], Fr[near]) < 2e-6 and _rel_l2(G[near], Gr[near]) < 2e-5


@pytest.mark.parametrize("kh", [60.0, 100.0, 1e-6])
def test_point_is_finite_where_sinh_and_cosh_overflow_and_at_tiny_kh(kh):
    V, W = _jets(1, 24, np.array([kh]))
    f, g = _point(V[0], W[0, 0], W[0, 1], SCALE)
    assert np.isfinite(f).all() and np.isfinite(g).all(), (kh, f, g)


def test_k_zero_gives_non_finite_values_that_propagate():
    V, W = _jets(1, 25)
    V[0, 5] = 0.0
    f, g = _point(V[0], W[0, 0], W[0, 1], SCALE)
    assert not np.isfinite(f[4]) and np.isfinite(f[:3]).all()


def test_terms_0_to_2_are_the_corrected_residuals_bit_for_bit():
    V, W = _jets(500, 26)
    s3 = (0.7, 1.3, 0.9)
    for v, w in zip(V, W):
        f5, g5 = _point(v, w[0], w[1], s3 + (0.0, 0.0))
        f3, g3 = _corrected_point(v, s3)
        assert np.array_equal(f5[:3], f3), (f5, f3)
        assert np.array_equal(g5, g3), (g5, g3)           # the two new terms at scale 0 add exact zeros


def test_point_without_scale_or_g_forms_the_fields_only_and_checks_the_wave():
    V, W = _jets(1, 27)
    f0, _ = _point(V[0], W[0, 0], W[0, 1], SCALE)
    f1, g1 = _point(V[0], W[0, 0], W[0, 1], None)
    assert np.array_equal(f0, f1) and np.all(g1 == 0.0)
    f2, _ = _point(V[0], W[0, 0], W[0, 1], SCALE, want_g=False)
    assert np.array_equal(f0, f2)
    lib = _lib.load()
    f = np.zeros(5, np.float32)
    for om, ga in ((0.0, 0.42), (-1.0, 0.42), (2.5, 0.0), (float("nan"), 0.42)):
        assert lib.pinn_pe_wave_point(V[0].ctypes.data_as(FP), om, ga, None, f.ctypes.data_as(FP), None) == ERR_INVALID
        assert "wave" in lib.pinn_last_error().decode()


def test_the_test_formula_is_the_packages():
    """pe_wave_util.wave_loss restates physics.physics_equation(corrected=True, wave_omega=) (it needs the fields apart)."""
    V, _ = _jets(50, 28)
    V = torch.tensor(V, dtype=torch.float64).reshape(-1, 3, 6)
    x = torch.zeros(50, 1, dtype=torch.float64, requires_grad=True)
    y = torch.zeros(50, 1, dtype=torch.float64, requires_grad=True)
    outs = [V[:, 0, r:r + 1] + V[:, 1, r:r + 1] * x + V[:, 2, r:r + 1] * y for r in range(6)]
    a = physics.physics_equation(x, y, *outs, corrected=True, wave_omega=1.7, wave_gamma=0.5)
    assert float(a.detach()) == pytest.approx(float(wave_loss(x, y, *outs, omega=1.7, gamma=0.5).detach()), rel=1e-14)
    assert float(physics.physics_equation_wave(x, y, *outs, 1.7, 0.5).detach()) == float(a.detach())      # plain tensors: the formula
    assert float(a.detach()) != pytest.approx(float(physics.physics_equation(x, y, *outs, corrected=True).detach()), rel=1e-3)
    with pytest.raises(PinnError, match="wave"):
        physics.physics_equation(x, y, *outs, wave_omega=1.7)                   # without corrected
    with pytest.raises(PinnError, match="wave"):
        physics.physics_equation(x, y, *outs, corrected=True, wave_omega=-1.0)
    with pytest.raises(PinnError, match="wave"):
        physics.physics_equation(x, y, *outs, corrected=True, wave_omega=1.0, nu=0.1)


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_flag_param_and_counts():
    d = NetDesc(2, 6, 10, 10, (0, 1))
    s = _spec(d, 2.5, 0.5)
    c = s.c_struct()
    assert s.corrected and s.wave and c.flags == 3 and c.residual_id == _lib.RES_PHYSICS_EQUATION
    assert c.param[0] == 2.5 and c.param[1] == 0.5
    assert s.n_terms == 5 and s.n_fields == 5 and s.coef_names == () and _lib.PEW_TERMS == 5
    plain = ResidualSpec.from_names("physics_equation", PE_IN, d.grad_cols, ROLES, corrected=True)
    assert not plain.wave and plain.c_struct().flags == 1 and plain.n_terms == 3 and plain.c_struct().param[0] == 25.5
    assert ResidualSpec.from_names("physics_equation", PE_IN, d.grad_cols, ROLES, corrected=True, wave_omega=2.5).wave_gamma == 0.42
    assert _lib.RES_TERMS == {1: 3, 2: 3, 3: 1, 4: 3}                          # (keyed by id: the count comes from the spec)
    with pytest.raises(PinnError, match="wave"):
        ResidualSpec.from_names("physics_equation", PE_IN, d.grad_cols, ROLES, wave_omega=2.5)           # without corrected
    with pytest.raises(PinnError, match="wave"):
        ResidualSpec("continuity_ftemp", (0, 1, 2), (0, 1), wave_omega=2.5)
    with pytest.raises(PinnError, match="wave"):
        ResidualSpec.from_names("physics_equation", PE_IN, d.grad_cols, ROLES, corrected=True, wave_omega=2.5, wave_gamma=0.0)
    with pytest.raises(PinnError, match="wave"):
        ResidualSpec.from_names("physics_equation", PE_IN, d.grad_cols, ROLES, corrected=True, wave_omega=2.5, nu=0.1)
    lib = _lib.load()
    assert "pinn_pe_wave_point" in _lib.exported_symbols() and lib.pinn_pe_wave_point.restype is C.c_int32
    assert lib.pinn_version() == _lib.ABI_VERSION == 4
    n = C.c_int32(-1)
    assert lib.pinn_residual_coef_count(2, 3, C.byref(n)) == 0 and n.value == 0


# ---- C-ABI validation and dispatch: no device, fake pointers -------------------------------------------------------------
_P = C.c_void_p(0x1000)


def _loss_calls(desc, cspec, n_cols=1):
    """Every loss entry that takes a spec, with fake non-NULL pointers and NO workspace (ws = NULL, ws_bytes = 0): a request
    an engine serves stops at that engine's workspace check, its first statement, with PINN_ERR_WORKSPACE; everything else
    is refused before.  N = 64 with n_res = 48 (or both terms on every point): no entry zeroes col_sums ahead of the check."""
    lib = _lib.load()
    d, s = desc.c_struct(), cspec
    oc = (C.c_int32 * 8)(0, 1, 2, 3, 4, 5, 0, 1)
    st = _lib.PinnAdamState(_P, _P, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None)
    lr = (C.c_double * 2)(1e-3, 1e-3)
    ws, big = None, 0
    calls = [
        ("pinn_residual_loss", lambda: lib.pinn_residual_loss(C.byref(d), C.byref(s), _P, _P, 64, _P, ws, big, None)),
        ("pinn_residual_loss_grad", lambda: lib.pinn_residual_loss_grad(C.byref(d), C.byref(s), _P, _P, _P, 64, _P, _P, ws, big, None)),
        ("pinn_residual_mse_loss_grad", lambda: lib.pinn_residual_mse_loss_grad(C.byref(d), C.byref(s), _P, _P, n_cols, oc, _P, _P, _P, 64, _P, _P,
                                                                                _P, ws, big, None)),
        ("pinn_residual_mse_split_loss_grad", lambda: lib.pinn_residual_mse_split_loss_grad(C.byref(d), C.byref(s), _P, _P, n_cols, oc, _P, _P, _P, 64,
                                                                                            48, _P, _P, _P, ws, big, None)),
        ("pinn_loss_grad_adam_step", lambda: lib.pinn_loss_grad_adam_step(C.byref(d), C.byref(s), _P, _P, n_cols, oc, _P, _P, _P, 64, 48, _P, _P, _P,
                                                                          C.byref(st), ws, big, None)),
        ("pinn_adam_loop", lambda: lib.pinn_adam_loop(C.byref(d), C.byref(s), _P, _P, n_cols, oc, _P, _P, _P, 64, 48, _P, _P, _P, C.byref(st), 2, lr,
                                                      ws, big, None)),
        ("pinn_lbfgs_loop", lambda: lib.pinn_lbfgs_loop(C.byref(d), C.byref(s), _P, _P, n_cols, oc, _P, _P, _P, 64, 48, 1, _P, 0, _P, 1 << 40, 1, None,
                                                        ws, big, None)),
    ]
    return [(name, fn(), lib.pinn_last_error().decode()) for name, fn in calls]


def _cspec(desc, flags=3, omega=2.5, gamma=0.42, residual_id=None):
    s = _spec(desc, inputs=("x", "y", "t") if desc.k == 3 else PE_IN).c_struct()
    s.flags, s.param[0], s.param[1] = flags, omega, gamma
    if residual_id is not None:
        s.residual_id = residual_id
    return s


@pytest.mark.parametrize("what,kw,word", [
    ("bit 1 without bit 0", dict(flags=2), "wave"),
    ("omega = 0", dict(omega=0.0), "wave"),
    ("omega < 0", dict(omega=-2.5), "wave"),
    ("omega NaN", dict(omega=float("nan")), "wave"),
    ("gamma = 0", dict(gamma=0.0), "wave"),
    ("private id 5", dict(residual_id=5), "residual_id"),
    ("private id 6", dict(residual_id=6), "residual_id"),
])
def test_abi_validation_before_any_device_work(what, kw, word):
    d = NetDesc(2, 6, 10, 10, (0, 1))
    for name, rc, msg in _loss_calls(d, _cspec(d, **kw)):
        assert rc == ERR_INVALID and word in msg, (what, name, rc, msg)
    lib = _lib.load()
    need = C.c_int64(-1)
    for q in ("fields", "residual2", "residual_coef", "residual_weighted"):
        rc = getattr(lib, f"pinn_query_{q}_workspace")(C.byref(d.c_struct()), C.byref(_cspec(d, **kw)), 64, C.byref(need))
        assert rc == ERR_INVALID and word in lib.pinn_last_error().decode(), (what, q, rc)


SHAPES = {"10x10": (2, 6, 10, 10), "3x24": (2, 6, 3, 24), "8x64": (2, 6, 8, 64), "3x100": (2, 6, 3, 100)}
ENGINES = {"AUTO": ENGINE_AUTO, "GENERIC": ENGINE_GENERIC, "FUSED": ENGINE_FUSED, "WIDE": ENGINE_WIDE, "FUSED_TILE": ENGINE_FUSED_TILE,
           "FUSED_COOP": ENGINE_FUSED_COOP, "FUSED_BATCH": ENGINE_FUSED_BATCH}
VARIANTS = {"tanh": {}, "leaky": dict(activation=ACT_LEAKY_RELU), "sine": dict(activation=ACT_SIN_TANH), "dropout": dict(dropout_p=0.25),
            "k3": dict(k3=True), "bf16": dict(precision=PREC_BF16)}


def _expected(shape, engine, variant):
    """The header's engine rule for a wave loss request: served by the "tile" kernel or by the "generic" engine, or "refused"."""
    width = SHAPES[shape][3]
    if variant == "bf16":
        return "refused"                                       # every descriptor whose engine comes out as WIDE
    if engine == "GENERIC":
        return "generic"                                       # any shape, tanh or LeakyReLU or sine, dropout, k = 2 or 3
    if engine == "AUTO" and variant in ("sine", "dropout"):
        return "generic"                                       # at every width
    if engine == "AUTO" and width > 64 and variant == "leaky":
        return "generic"                                       # (AUTO picks the generic engine for a wide LeakyReLU network)
    if engine == "WIDE" or width > 64:
        return "refused"
    if engine in ("FUSED_COOP", "FUSED_BATCH"):
        return "refused"                                       # tile-kernel instances only
    if variant in ("sine", "dropout", "leaky", "k3"):
        return "refused"                                       # on FUSED; AUTO picks FUSED for LeakyReLU and k = 3 at these widths
    return "tile"


def _desc(shape, engine, variant):
    d_in, d_out, L, W = SHAPES[shape]
    kw = dict(VARIANTS[variant])
    if kw.pop("k3", False):
        return NetDesc(3, d_out, L, W, (0, 1, 2), engine=ENGINES[engine])
    return NetDesc(d_in, d_out, L, W, (0, 1), engine=ENGINES[engine], **kw)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dispatch_walk_descriptor_by_engine(shape, variant):
    """Every loss entry, for every engine value: served requests reach an engine's workspace check, refused ones say "wave"
    and name GENERIC (unless GENERIC itself was asked for); the same descriptor with flags = 1 never says "wave"."""
    for engine in ENGINES:
        desc = _desc(shape, engine, variant)
        want = _expected(shape, engine, variant)
        for name, rc, msg in _loss_calls(desc, _cspec(desc)):
            ctx = (shape, variant, engine, want, name, rc, msg)
            if variant == "dropout" and name == "pinn_lbfgs_loop":        # the device L-BFGS loop takes no dropout, whatever the residual
                assert rc == ERR_UNSUPPORTED and "dropout" in msg, ctx
            elif want == "generic" and name in ("pinn_loss_grad_adam_step", "pinn_adam_loop"):   # the folded update is the fused engine's
                assert rc == ERR_UNSUPPORTED and "fused engine" in msg, ctx
            elif want != "refused":
                assert rc == ERR_WORKSPACE, ctx
            else:
                assert rc == ERR_UNSUPPORTED and "wave" in msg, ctx
                if engine != "GENERIC":
                    assert "GENERIC" in msg, ctx
        for name, rc, msg in _loss_calls(desc, _cspec(desc, flags=1)):
            assert "wave" not in msg, (shape, variant, engine, name, rc, msg)


def test_the_eighth_fidelity_column_is_refused_on_the_fused_engine_only():
    for shape in ("10x10", "3x24", "8x64"):
        d = _desc(shape, "AUTO", "tanh")
        for name, rc, msg in _loss_calls(d, _cspec(d), n_cols=7):
            assert rc == ERR_WORKSPACE, (shape, name, rc, msg)
        for name, rc, msg in _loss_calls(d, _cspec(d), n_cols=8):
            if name in ("pinn_residual_loss", "pinn_residual_loss_grad"):
                assert rc == ERR_WORKSPACE, (shape, name, rc, msg)                 # no columns in these
            else:
                assert rc == ERR_UNSUPPORTED and "wave" in msg and "column" in msg and "GENERIC" in msg, (shape, name, rc, msg)
        g = _desc(shape, "GENERIC", "tanh")
        for name, rc, msg in _loss_calls(g, _cspec(g), n_cols=8):              # (the folded update is the fused engine's)
            assert rc == (ERR_UNSUPPORTED if name in ("pinn_loss_grad_adam_step", "pinn_adam_loop") else ERR_WORKSPACE), (shape, name, rc, msg)
            assert "wave" not in msg and "column" not in msg, (shape, name, rc, msg)
        for name, rc, msg in _loss_calls(d, _cspec(d, flags=1), n_cols=8):
            assert rc == ERR_WORKSPACE, (shape, name, rc, msg)                     # the corrected residual keeps its eight


def test_out_of_scope_entries_refuse_with_the_word_wave():
    lib = _lib.load()
    d = NetDesc(2, 6, 10, 10, (0, 1))
    cd, s = d.c_struct(), _cspec(d)
    need = C.c_int64(-1)
    oc = (C.c_int32 * 2)(0, 1)
    st = _lib.PinnAdamState(_P, _P, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None)
    lr = (C.c_double * 2)(1e-3, 1e-3)

    def refused(what, rc):
        msg = lib.pinn_last_error().decode()
        assert rc == ERR_UNSUPPORTED and "wave" in msg, (what, rc, msg)

    for q in ("residual2", "residual_coef", "residual_weighted"):
        refused(q, getattr(lib, f"pinn_query_{q}_workspace")(C.byref(cd), C.byref(s), 64, C.byref(need)))
    refused("residual2", lib.pinn_residual2_loss_grad(C.byref(cd), C.byref(s), 0.01, _P, _P, _P, 64, _P, _P, _P, None, 0, None))
    refused("coef", lib.pinn_residual_coef_loss_grad(C.byref(cd), C.byref(s), _P, _P, _P, _P, 64, _P, _P, _P, None, 0, None))
    refused("weighted", lib.pinn_residual_weighted_loss_grad(C.byref(cd), C.byref(s), _P, _P, 1, _P, _P, 64, _P, _P, _P, None, 0, None))
    f = np.zeros(3, np.float32)
    refused("residual2_point", lib.pinn_residual2_point(2, 3, 0.01, f.ctypes.data_as(FP), f.ctypes.data_as(FP), None, f.ctypes.data_as(FP), None, None))
    for group in ("coef", "weights"):
        ex = _lib.PinnAdamExtras()
        if group == "coef":
            ex.coef, ex.coef_m, ex.coef_v, ex.coef_grad = 0x1000, 0x1000, 0x1000, 0x1000
        else:
            ex.point_w, ex.w_rows = 0x1000, 1
        refused("ext query " + group, lib.pinn_query_adam_ext_workspace(C.byref(cd), C.byref(s), C.byref(ex), 64, 0, C.byref(need)))
        refused("ext " + group, lib.pinn_adam_loop_ext(C.byref(cd), C.byref(s), _P, _P, _P, 0, 0, oc, _P, _P, _P, 64, _P, _P, _P, C.byref(st),
                                                      C.byref(ex), 2, lr, lr, lr, None, 0, None))
    refused("balanced query", lib.pinn_query_adam_balanced_workspace(C.byref(cd), C.byref(s), 64, 8, C.byref(need)))
    bal = _lib.PinnBalance(1, 10, 0, 0.1, 0x1000, None, None, None)
    refused("balanced", lib.pinn_adam_loop_balanced(C.byref(cd), C.byref(s), _P, _P, _P, 8, 2, oc, _P, _P, _P, 64, _P, _P, _P, C.byref(st),
                                                    C.byref(bal), 2, lr, None, 0, None))
    refused("ensemble", lib.pinn_ensemble_loss_grad(C.byref(cd), C.byref(s), 3, _P, _P, 0, oc, _P, _P, _P, 64, 64, 0, _P, _P, _P, None, 0, None))
    refused("ensemble adam", lib.pinn_ensemble_adam_step(C.byref(cd), C.byref(s), 3, _P, _P, 0, oc, _P, _P, _P, 64, 64, 0, _P, _P, _P, C.byref(st),
                                                         None, 0, None))
    refused("ensemble lbfgs", lib.pinn_ensemble_lbfgs_loop(C.byref(cd), C.byref(s), 3, _P, _P, 0, oc, _P, _P, _P, 64, 64, 0, 1, _P, 0, 10, _P,
                                                           1 << 40, 1, None, None, 0, None))


def _fields_query(desc, cspec):
    lib = _lib.load()
    need = C.c_int64(-1)
    rc = lib.pinn_query_fields_workspace(C.byref(desc.c_struct()), C.byref(cspec), 64, C.byref(need))
    return rc, need.value, lib.pinn_last_error().decode()


def test_fields_query_tile_instances_for_tanh_else_staged_or_refused():
    d = NetDesc(2, 6, 10, 10, (0, 1))
    tile, staged = _fields_query(d, _cspec(d)), _fields_query(d.with_(engine=ENGINE_GENERIC), _cspec(d))
    assert tile[0] == 0 and staged[0] == 0 and staged[1] > tile[1] > 0
    assert tile[1] == _fields_query(d.with_(engine=ENGINE_FUSED), _cspec(d))[1]
    leaky = d.with_(activation=ACT_LEAKY_RELU)                                # AUTO: staged; FUSED: refused
    assert _fields_query(leaky, _cspec(leaky))[0] == 0 and _fields_query(leaky, _cspec(leaky))[1] > tile[1]
    rc, _, msg = _fields_query(leaky.with_(engine=ENGINE_FUSED), _cspec(leaky))
    assert rc == ERR_UNSUPPORTED and "wave" in msg
    k3 = NetDesc(3, 6, 3, 20, (0, 1, 2))
    rc, _, msg = _fields_query(k3, _cspec(k3))
    assert rc == ERR_UNSUPPORTED and "wave" in msg                            # fields need k = the residual's two directions
    wide = NetDesc(2, 6, 3, 100, (0, 1))
    assert _fields_query(wide, _cspec(wide))[0] == 0


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


def test_trainer_keywords_and_config_keys():
    assert not _pinn(_cfg(ROLES), corrected=True).spec.wave
    tr = _pinn(_cfg(ROLES), corrected=True, wave_period=8.0)
    assert tr.spec.wave and tr.spec.wave_omega == pytest.approx(2 * math.pi / 8.0) and tr.spec.wave_gamma == 0.42
    assert tr.spec.n_terms == 5 and tr._res_sums.numel() == 5 and tr.spec.c_struct().flags == 3
    tr = _pinn(_cfg(ROLES, corrected_radiation_stress=True, wave_period=5.0, wave_gamma=0.6))
    assert tr.wave_period == 5.0 and tr.spec.wave_omega == pytest.approx(2 * math.pi / 5.0) and tr.spec.wave_gamma == 0.6
    c = tr.spec.c_struct()
    assert c.flags == 3 and c.param[0] == pytest.approx(2 * math.pi / 5.0, rel=1e-7) and c.param[1] == pytest.approx(0.6, rel=1e-7)
    assert _pinn(_cfg(ROLES, corrected_radiation_stress=True, wave_period=5.0), wave_period=4.0).wave_period == 4.0   # the argument wins
    # the five term weights default to 1: every term's scale is weight_res / N
    from pinn_depthestimation_amd.trainer import loss_arithmetic
    res_scale = loss_arithmetic(tr.config, tr.spec, 0, 0, 32, "cpu")[3]
    assert res_scale.tolist() == [1.0 / 32] * 5
    for kw, cfg in ((dict(wave_period=8.0), _cfg(ROLES)),                                               # without corrected
                    (dict(), _cfg(ROLES, wave_period=8.0)),
                    (dict(corrected=True, wave_period=-1.0), _cfg(ROLES)),
                    (dict(corrected=True, wave_period=8.0, wave_gamma=0.0), _cfg(ROLES)),
                    (dict(corrected=True, wave_period=8.0, eddy_viscosity=0.1), _cfg(ROLES)),
                    (dict(corrected=True, wave_period=8.0, coefficients={"Cd": 0.01}), _cfg(ROLES)),
                    (dict(corrected=True, wave_period=8.0, residual_weights=np.ones(32, np.float32)), _cfg(ROLES)),
                    (dict(corrected=True, wave_period=8.0, self_adaptive=True), _cfg(ROLES))):
        with pytest.raises(PinnError, match="wave"):
            _pinn(cfg, **kw)
    with pytest.raises(PinnError, match="wave"):
        _pinn(_cfg(("U", "V", "h")), residual="continuity_ftemp", wave_period=8.0)


def test_refusal_helpers_name_the_wave_closure():
    from pinn_depthestimation_amd import trainer as T
    assert "wave" in T.coefficient_refusal("physics_equation", {"Cd": 0.01}, (), corrected=True, wave=True)
    assert "wave" in T.weighted_refusal(residual_weights=True, corrected=True, wave=True)
    assert "wave" in T.balance_refusal("max_mean", wave=True)
    assert "wave" in T.wave_refusal(8.0, 0.42, "physics_equation", True, eddy_viscosity=0.1)
    assert T.wave_refusal(None, 0.42, "Navier_Stokes", False) is None and T.wave_refusal(8.0, 0.42, "physics_equation", True) is None
    # ... and without it they say what they said
    assert "wave" not in T.coefficient_refusal("physics_equation", {"Cd": 0.01}, (), corrected=True)
    assert "wave" not in T.weighted_refusal(residual_weights=True, corrected=True)
    assert T.balance_refusal("max_mean") is None


def test_ensemble_and_tester_read_the_config_keys():
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.ensemble import EnsemblePINN
    from pinn_depthestimation_amd.inference import Tester
    cfg = _cfg(ROLES, corrected_radiation_stress=True, wave_period=5.0, wave_gamma=0.6)
    with pytest.raises(PinnError, match="wave"):
        EnsemblePINN(None, None, np.zeros((32, 2), np.float32), cfg, members=2, device="cpu")
    model = DNN([2, 10, 10, 6], 0.0, "xavier")
    t = Tester(model, cfg, device="cpu")
    assert t.corrected and t.wave_period == 5.0 and t.wave_gamma == 0.6 and t.wave_omega == pytest.approx(2 * math.pi / 5.0)
    t = Tester(model, _cfg(ROLES), device="cpu", corrected=True, wave_period=4.0)
    assert t.wave_period == 4.0 and t.wave_gamma == 0.42
    assert Tester(model, _cfg(ROLES), device="cpu", corrected=True).wave_period is None
    t = Tester(model, _cfg(ROLES, corrected_radiation_stress=True), device="cpu", wave_period=4.0)     # the key counts with the argument too
    assert t.corrected and t.wave_period == 4.0
    with pytest.raises(PinnError, match="wave"):
        Tester(model, _cfg(ROLES), device="cpu", wave_period=4.0)

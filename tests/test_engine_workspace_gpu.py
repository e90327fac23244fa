"""Engine's workspace cache on the device: every kind of workspace is at least what its query answers, is handed out again
as the same tensor while it fits, only grows, and asks the library once per need key; and the loss entries check a
caller's sums buffer before anything is launched."""
import collections
import ctypes as C

import pytest
import torch

from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd import _lib
from pinn_depthestimation_amd._lib import PinnError

pytestmark = pytest.mark.gpu

N_SMALL, N_BIG = 33, 1000      # a partial 16-point tile; more than one workgroup
# 3 inputs, 6 outputs.  physics_equation differentiates two inputs (x, y) and Navier_Stokes three (t, x, y), and every
# residual entry wants the network's directions to be the residual's: the physics_equation roles run on grad_cols (1, 2),
# grad_cols (0, 1, 2) with the Navier_Stokes roles
NETS = {"physics_equation": ((1, 2), ("h", "U", "V", "eta_mean", "Hrms", "k"), 0.002),
        "Navier_Stokes": ((0, 1, 2), ("h", "z", "u", "v", "p", "q"), 0.78)}


class Counting:
    """eng.lib with a count of the calls of every symbol."""

    def __init__(self, lib):
        self._lib, self.count = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def f(*a):
            self.count[name] += 1
            return fn(*a)
        return f


def _engine(width, residual="physics_equation"):
    grad_cols, out, _ = NETS[residual]
    desc = NetDesc(3, 6, 2, width, grad_cols)
    eng = Engine(desc, "cuda")
    eng.lib = Counting(eng.lib)
    return eng, ResidualSpec.from_names(residual, ("t", "x", "y"), desc.grad_cols, out)


def _direct(eng, symbol, *args):
    """What the library's own query answers, asked under the engine's device, past the engine and its counting."""
    need = C.c_int64()
    with torch.cuda.device(eng._index()):
        assert getattr(_lib.load(), symbol)(C.byref(eng._d()), *args, C.byref(need)) == 0, symbol
    return need.value


def _tensors(eng, spec, N, seed=3):
    g = torch.Generator().manual_seed(seed)
    P, z = eng.n_params, lambda *s: torch.zeros(*s, device="cuda")
    theta = (torch.randn(P, generator=g) * 0.1)
    theta[-6] = 0.75       # the bias of h: a depth away from zero
    return dict(theta=theta.cuda(), X=(torch.rand(N, 3, generator=g) * 2 - 1).cuda(), grad=z(P), m=z(P), v=z(P),
                scale=torch.full((spec.n_terms,), 1.0 / N, device="cuda"), ts=z(spec.n_terms))


def _ext(eng, spec, kind, N):
    """One iteration of adam_loop_ext of the kind; returns (the workspace it ran in, the bytes its query answers)."""
    t, z = _tensors(eng, spec, N), lambda *s: torch.zeros(*s, device="cuda")
    ex = _lib.PinnAdamExtras()
    if kind == "coef":
        kw = dict(coef=torch.tensor([NETS[spec.name][2]], device="cuda"), coef_m=z(1), coef_v=z(1), coef_grad=z(1), lr_coef=[1e-4])
        ex.coef, ex.coef_m, ex.coef_v, ex.coef_grad = (kw[k].data_ptr() for k in ("coef", "coef_m", "coef_v", "coef_grad"))
    else:
        kw = dict(point_w=torch.ones(1, N, device="cuda"))
        ex.point_w, ex.w_rows = kw["point_w"].data_ptr(), 1
    assert eng.adam_loop_ext(spec, t["scale"], t["theta"], t["X"], t["grad"], t["m"], t["v"], 1, [1e-4], term_sums=t["ts"], **kw), \
        eng.last_error()
    torch.cuda.synchronize()
    return eng._ws["adamext"], _direct(eng, "pinn_query_adam_ext_workspace", C.byref(spec.c_struct()), C.byref(ex), N, 0)


@pytest.mark.parametrize("residual", sorted(NETS))
@pytest.mark.parametrize("width", [16, 64])
def test_every_workspace_is_sized_by_its_query_reused_and_only_grows(width, residual):
    eng, spec = _engine(width, residual)
    s = C.byref(spec.c_struct())
    kinds = {      # name -> (the engine's way to the workspace of N points and the bytes its query answers, the query symbol)
        "workspace": (lambda N: (eng.workspace(N), _direct(eng, "pinn_query_workspace", N)), "pinn_query_workspace"),
        "jet2": (lambda N: (eng.jet2_workspace(N), _direct(eng, "pinn_query_jet2_workspace", N)), "pinn_query_jet2_workspace"),
        "fields": (lambda N: (eng.fields_workspace(spec, N), _direct(eng, "pinn_query_fields_workspace", s, N)),
                   "pinn_query_fields_workspace"),
        "coef": (lambda N: (eng.residual_coef_workspace(spec, N), _direct(eng, "pinn_query_residual_coef_workspace", s, N)),
                 "pinn_query_residual_coef_workspace"),
        "weighted": (lambda N: (eng.residual_weighted_workspace(spec, N), _direct(eng, "pinn_query_residual_weighted_workspace", s, N)),
                     "pinn_query_residual_weighted_workspace"),
        "res2": (lambda N: (eng.residual2_workspace(spec, N), _direct(eng, "pinn_query_residual2_workspace", s, N)),
                 "pinn_query_residual2_workspace"),
        "ensemble": (lambda N: (eng.ensemble_workspace(2, N), _direct(eng, "pinn_ensemble_query_workspace", 2, N)),
                     "pinn_ensemble_query_workspace"),
        "ext coef": (lambda N: _ext(eng, spec, "coef", N), "pinn_query_adam_ext_workspace"),
        "ext weighted": (lambda N: _ext(eng, spec, "w", N), "pinn_query_adam_ext_workspace"),
    }
    keys = collections.Counter()
    for name, (get, symbol) in kinds.items():
        small, need = get(N_SMALL)
        assert small.dtype == torch.uint8 and small.device == eng.device and small.numel() >= max(need, 256), name
        assert get(N_SMALL)[0] is small, name                        # a call that fits: the same object
        big, need = get(N_BIG)
        assert big.numel() >= max(need, small.numel()), name         # grows or keeps
        assert (big is small) == (big.numel() == small.numel()), name
        assert get(N_SMALL)[0] is big and get(N_BIG)[0] is big, name      # the small request afterwards gets the grown one
        keys[symbol] += 2                                            # two need keys per kind: the two N
    for symbol, n in keys.items():
        assert eng.lib.count[symbol] == n, (symbol, dict(eng.lib.count))
    # the kinds keep apart: one buffer each (the two ext kinds share "adamext")
    bufs = [eng._ws[k] for k in (eng.desc.engine, ("jet2", 0), ("fields", 0), ("coef", 0), ("weighted", 0), ("res2", 0), "ens", "adamext")]
    assert len({b.data_ptr() for b in bufs}) == len(bufs) == len(eng._ws)


def test_a_wrong_sums_buffer_is_refused_before_anything_is_launched():
    eng, spec = _engine(16)
    t, z = _tensors(eng, spec, N_SMALL), lambda *s: torch.zeros(*s, device="cuda")
    nt, T, cs = spec.n_terms, z(N_SMALL, 2), z(2)      # (two fidelity columns: a strided buffer of one element is contiguous)
    bad = {"one more": lambda n: z(n + 1), "float64": lambda n: z(n).double(), "strided": lambda n: z(2 * n)[::2],
           "off the device": lambda n: torch.zeros(n)}
    for why, make in bad.items():
        calls = {
            "pinn_residual_loss_grad": [lambda: eng.residual_loss_grad(spec, t["scale"], t["theta"], t["X"], t["grad"], sums=make(nt))],
            "pinn_mse_loss_grad": [lambda: eng.mse_loss_grad(t["theta"], t["X"], T, [0, 1], cs, t["grad"], sums=make(2))],
            "pinn_residual_mse_loss_grad": [
                lambda: eng.residual_mse_loss_grad(spec, t["scale"], T, [0, 1], cs, t["theta"], t["X"], t["grad"], term_sums=make(nt)),
                lambda: eng.residual_mse_loss_grad(spec, t["scale"], T, [0, 1], cs, t["theta"], t["X"], t["grad"], col_sums=make(2))],
            "pinn_residual_mse_split_loss_grad": [
                lambda: eng.residual_mse_split_loss_grad(spec, t["scale"], T[:3], [0, 1], cs, t["theta"], t["X"], N_SMALL - 3, t["grad"],
                                                         term_sums=make(nt)),
                lambda: eng.residual_mse_split_loss_grad(spec, t["scale"], T[:3], [0, 1], cs, t["theta"], t["X"], N_SMALL - 3, t["grad"],
                                                         col_sums=make(2))],
        }
        for symbol, fns in calls.items():
            for fn in fns:
                with pytest.raises(PinnError, match="sums"):
                    fn()
            assert eng.lib.count[symbol] == 0, (why, symbol)
    # ... and the right ones go through
    eng.residual_loss_grad(spec, t["scale"], t["theta"], t["X"], t["grad"], sums=z(nt))
    eng.residual_mse_split_loss_grad(spec, t["scale"], T[:3], [0, 1], cs, t["theta"], t["X"], N_SMALL - 3, t["grad"], term_sums=z(nt),
                                     col_sums=z(2))
    torch.cuda.synchronize()
    assert eng.lib.count["pinn_residual_loss_grad"] == 1 and eng.lib.count["pinn_residual_mse_split_loss_grad"] == 1

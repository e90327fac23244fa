"""The ensemble entries without a GPU: the symbols, everything the C-ABI decides before device work (M, the refusals, the
arguments — pinn_hip.h, "ensembles"), the launch plan (host logic) and EnsemblePINN's seed handling."""
import ctypes as C
import os

import pytest
import torch

from pinn_depthestimation_amd import NetDesc, PinnError, ResidualSpec, _lib
from pinn_depthestimation_amd.dnn import init_flat_params
from pinn_depthestimation_amd.ensemble import DEFAULT_SEED, init_ensemble_params, member_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = None
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
ENTRIES = ("pinn_ensemble_query_workspace", "pinn_ensemble_plan", "pinn_ensemble_loss_grad", "pinn_ensemble_adam_step",
           "pinn_ensemble_adam_loop")
FAKE = C.c_void_p(0x1000)        # never dereferenced: validation fails first

PE = dict(d_in=2, d_out=6, n_hidden=10, width=10, grad_cols=(0, 1))
PE_SPEC = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ("h", "U", "V", "eta_mean", "Hrms", "k"))
NS = dict(d_in=3, d_out=4, n_hidden=8, width=64, grad_cols=(0, 1, 2))
NS_SPEC = ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), (0, 1, 2), ("h", "z", "u", "v"))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def err(lib):
    return lib.pinn_last_error().decode()


def loss_grad(lib, desc, spec, M, N, n_res, n_cols=0, flags=0, params=FAKE, X=FAKE, T=FAKE, ws_bytes=1 << 40):
    oc = (C.c_int32 * 8)(*range(8))
    return lib.pinn_ensemble_loss_grad(C.byref(desc.c_struct()), C.byref(spec.c_struct()), M, FAKE, T, n_cols, oc, FAKE, params, X, N,
                                       n_res, flags, FAKE, FAKE, FAKE, FAKE, ws_bytes, NULL)


def test_the_entries_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    for name in ENTRIES:
        assert f"int32_t {name}(" in header, name
        assert name in _lib.exported_symbols()
        assert getattr(lib, name).restype is C.c_int32
    for macro, value in (("PINN_ENSEMBLE_OWN_X", _lib.ENSEMBLE_OWN_X), ("PINN_ENSEMBLE_OWN_T", _lib.ENSEMBLE_OWN_T),
                         ("PINN_ENSEMBLE_MAX_MEMBERS", _lib.ENSEMBLE_MAX_MEMBERS)):
        assert f"#define {macro} {value}" in header
    assert lib.pinn_version() == 4          # added under ABI version 4


def test_member_count_is_validated_first(lib):
    need, gx, lds = C.c_int64(), C.c_int32(), C.c_int32()
    d = NetDesc(**PE)
    for M in (0, -3, 65536):
        assert lib.pinn_ensemble_query_workspace(C.byref(d.c_struct()), M, 255, C.byref(need)) == INVALID and "M =" in err(lib)
        assert lib.pinn_ensemble_plan(C.byref(d.c_struct()), M, 255, C.byref(gx), C.byref(lds)) == INVALID
        assert loss_grad(lib, d, PE_SPEC, M, 255, 243, 6) == INVALID and "M =" in err(lib)
    for M in (1, 65535):
        assert lib.pinn_ensemble_query_workspace(C.byref(d.c_struct()), M, 255, C.byref(need)) == OK, err(lib)
        assert need.value > 0
    assert lib.pinn_ensemble_query_workspace(C.byref(d.c_struct()), 3, 0, C.byref(need)) == INVALID
    assert lib.pinn_ensemble_query_workspace(C.byref(d.c_struct()), 3, 255, NULL) == INVALID
    assert lib.pinn_ensemble_plan(C.byref(d.c_struct()), 3, 255, NULL, C.byref(lds)) == INVALID
    assert lib.pinn_ensemble_query_workspace(NULL, 3, 255, C.byref(need)) == INVALID and "desc is NULL" in err(lib)


REFUSED = [
    ("generic", dict(PE, engine=_lib.ENGINE_GENERIC), PE_SPEC, "GENERIC"),
    ("wide", dict(NS, width=128, engine=_lib.ENGINE_WIDE), NS_SPEC, "WIDE"),
    ("coop", dict(NS, engine=_lib.ENGINE_FUSED_COOP), NS_SPEC, "FUSED_COOP"),
    ("batch", dict(PE, engine=_lib.ENGINE_FUSED_BATCH), PE_SPEC, "FUSED_BATCH"),
    ("bf16", dict(NS, width=128, precision=_lib.PREC_BF16), NS_SPEC, "bf16"),
    ("width", dict(NS, width=65), NS_SPEC, "width above 64"),
    ("leaky", dict(PE, activation=_lib.ACT_LEAKY_RELU), PE_SPEC, "LeakyReLU"),
    ("dropout", dict(NS, dropout_p=0.1), NS_SPEC, "dropout"),
    ("k0", dict(PE, grad_cols=()), None, "k must be 2 or 3"),
    ("k1", dict(PE, grad_cols=(0,)), None, "k must be 2 or 3"),
]


@pytest.mark.parametrize("name,kw,spec,what", REFUSED, ids=[r[0] for r in REFUSED])
def test_descriptors_without_an_ensemble_kernel_are_refused_by_every_entry(lib, name, kw, spec, what):
    d = NetDesc(**kw)
    need, gx, lds = C.c_int64(), C.c_int32(), C.c_int32()
    assert lib.pinn_ensemble_query_workspace(C.byref(d.c_struct()), 3, 255, C.byref(need)) == UNSUPPORTED
    assert what in err(lib), err(lib)
    assert lib.pinn_ensemble_plan(C.byref(d.c_struct()), 3, 255, C.byref(gx), C.byref(lds)) == UNSUPPORTED and what in err(lib)
    # the calls refuse before they look at the spec's roles or at a pointer: NULL arrays, still UNSUPPORTED
    sp = spec if spec is not None else PE_SPEC
    assert loss_grad(lib, d, sp, 3, 255, 255, params=NULL, X=NULL) == UNSUPPORTED and what in err(lib)
    st = _lib.PinnAdamState(FAKE, FAKE, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None)
    oc = (C.c_int32 * 8)(*range(8))
    head = (C.byref(d.c_struct()), C.byref(sp.c_struct()), 3, FAKE, FAKE, 0, oc, FAKE, FAKE, FAKE, 255, 255, 0, FAKE, FAKE, FAKE, C.byref(st))
    assert lib.pinn_ensemble_adam_step(*head, FAKE, 1 << 40, NULL) == UNSUPPORTED and what in err(lib)
    assert lib.pinn_ensemble_adam_loop(*head, 2, (C.c_double * 2)(1e-3, 1e-3), FAKE, 1 << 40, NULL) == UNSUPPORTED and what in err(lib)


def test_request_level_refusals(lib):
    # the corrected radiation stress
    corrected = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ("h", "U", "V", "eta_mean", "Hrms", "k"), corrected=True)
    assert loss_grad(lib, NetDesc(**PE), corrected, 3, 255, 243, 6) == UNSUPPORTED and "corrected" in err(lib)
    # the split request at padded width 64 (hidden width 33..64); the other two meanings of n_res are served there
    for width in (33, 64):
        d = NetDesc(**dict(NS, width=width))
        assert loss_grad(lib, d, NS_SPEC, 3, 255, 243, 2) == UNSUPPORTED and "split" in err(lib)
        assert loss_grad(lib, d, NS_SPEC, 3, 255, 255, 2, params=NULL) == INVALID          # past the refusals: the NULL array
        assert loss_grad(lib, d, NS_SPEC, 3, 255, -1, 2, params=NULL) == INVALID
    assert loss_grad(lib, NetDesc(**dict(NS, width=32)), NS_SPEC, 3, 255, 243, 2, params=NULL) == INVALID


def test_argument_validation_returns_before_any_launch(lib):
    d = NetDesc(**PE)
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 6, params=NULL) == INVALID and "NULL pointer" in err(lib)
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 6, X=NULL) == INVALID
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 6, T=NULL) == INVALID               # fidelity points without targets
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 256, 6) == INVALID and "n_res=256 exceeds N=255" in err(lib)
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 0) == INVALID and "n_res must equal N" in err(lib)
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 9) == INVALID and "n_cols=9" in err(lib)
    assert loss_grad(lib, d, PE_SPEC, 3, 0, 0, 6) == INVALID
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 6, flags=4) == INVALID and "flags" in err(lib)
    assert lib.pinn_ensemble_loss_grad(C.byref(d.c_struct()), NULL, 3, FAKE, FAKE, 0, NULL, FAKE, FAKE, FAKE, 255, 255, 0, FAKE, FAKE,
                                       FAKE, FAKE, 1 << 40, NULL) == INVALID and "spec is NULL" in err(lib)
    bad = ResidualSpec("physics_equation", (0, 1, 2, 3, 4, 9), (0, 1))
    assert loss_grad(lib, d, bad, 3, 255, 255) == INVALID and "outside the 6 output columns" in err(lib)
    # a workspace smaller than the query's answer, or none
    need = C.c_int64()
    assert lib.pinn_ensemble_query_workspace(C.byref(d.c_struct()), 3, 255, C.byref(need)) == OK
    assert loss_grad(lib, d, PE_SPEC, 3, 255, 243, 6, ws_bytes=need.value - 1) == WORKSPACE and str(need.value) in err(lib)
    # the Adam entries: a state without moments, a step count below one, loss rows without their output, no schedule
    oc = (C.c_int32 * 8)(*range(8))
    head = (C.byref(d.c_struct()), C.byref(PE_SPEC.c_struct()), 3, FAKE, FAKE, 6, oc, FAKE, FAKE, FAKE, 255, 243, 0, FAKE, FAKE, FAKE)
    assert lib.pinn_ensemble_adam_step(*head, NULL, FAKE, 1 << 40, NULL) == INVALID
    for st in (_lib.PinnAdamState(None, FAKE, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None),
               _lib.PinnAdamState(FAKE, FAKE, 0, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None),
               _lib.PinnAdamState(FAKE, FAKE, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 3, FAKE, None),
               _lib.PinnAdamState(FAKE, FAKE, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 9, FAKE, FAKE)):
        assert lib.pinn_ensemble_adam_step(*head, C.byref(st), FAKE, 1 << 40, NULL) == INVALID
    ok = _lib.PinnAdamState(FAKE, FAKE, 1, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None, None)
    assert lib.pinn_ensemble_adam_loop(*head, C.byref(ok), 2, NULL, FAKE, 1 << 40, NULL) == INVALID
    assert lib.pinn_ensemble_adam_loop(*head, C.byref(ok), -1, (C.c_double * 1)(1e-3), FAKE, 1 << 40, NULL) == INVALID
    assert lib.pinn_ensemble_adam_loop(*head, C.byref(ok), 0, (C.c_double * 1)(1e-3), FAKE, 1 << 40, NULL) == OK      # nothing to do


def plan(lib, kw, M, N):
    gx, lds, need = C.c_int32(), C.c_int32(), C.c_int64()
    d = NetDesc(**kw).c_struct()
    assert lib.pinn_ensemble_plan(C.byref(d), M, N, C.byref(gx), C.byref(lds)) == OK, err(lib)
    assert lib.pinn_ensemble_query_workspace(C.byref(d), M, N, C.byref(need)) == OK
    return gx.value, lds.value, need.value


def test_the_plan_clamps_the_grid_and_sizes_the_workspace_from_it(lib):
    """Without a device the library plans for 256 CUs (pinn_hip.h).  16 tiles are 4 workgroups of 4 waves; the narrow shapes
    run 2 workgroups per CU, so the cap is 512 workgroups: gx = min(4, max(1, 512 / M))."""
    for M, want in ((1, 4), (3, 4), (128, 4), (129, 3), (256, 2), (300, 1), (512, 1), (513, 1), (65535, 1)):
        gx, lds, _ = plan(lib, PE, M, 255)
        assert gx == want and lds == 1, (M, gx, lds)
    assert plan(lib, PE, 5, 16)[0] == 1                       # one tile: one workgroup
    # 8 x 64 keeps its gradient copy in LDS and fills it: one workgroup per CU, cap 256
    assert [plan(lib, NS, M, 243)[0] for M in (1, 64, 65, 128, 300)] == [4, 4, 3, 2, 1]
    # 40 x 20: the padded gradient (40 layers of 32 x 32) does not fit LDS — the copies live in the workspace
    co = dict(d_in=2, d_out=3, n_hidden=40, width=20, grad_cols=(0, 1))
    gx, lds, need = plan(lib, co, 3, 100)
    assert lds == 0 and gx == 2
    PP = (32 * 16 + 39 * 32 * 32 + 16 * 32) + (40 * 32 + 16)
    assert need >= 3 * gx * PP * 4 + 2 * 3 * (PP - 40 * 32 - 16) * 4       # the members' gradient copies + packed W, W^T
    # the workspace grows with M while gx holds, and not beyond what the clamped grid needs
    a, b = plan(lib, PE, 4, 255)[2], plan(lib, PE, 8, 255)[2]
    assert a < b <= 2 * a
    assert plan(lib, PE, 512, 255)[2] < 2 * plan(lib, PE, 128, 255)[2]      # gx 4 -> 1: a quarter of the slots per member


def test_member_seeds_and_initial_rows():
    assert member_seeds(3) == [DEFAULT_SEED, DEFAULT_SEED + 1, DEFAULT_SEED + 2]
    assert member_seeds(2, (7, 9)) == [7, 9]
    for bad in ((4, (1, 2, 3)), (2, (5, 5)), (0, None)):
        with pytest.raises(PinnError):
            member_seeds(*bad)
    layers = [2] + [10] * 10 + [6]
    seeds = member_seeds(4, (11, 12, 13, 99))
    theta = init_ensemble_params(layers, "xavier", seeds)
    assert theta.shape == (4, NetDesc(**PE).n_params) and theta.dtype == torch.float32
    for i, s in enumerate(seeds):
        assert torch.equal(theta[i], init_flat_params(layers, "xavier", torch.Generator().manual_seed(s)))
    for i in range(4):
        for j in range(i):
            assert not torch.equal(theta[i], theta[j])
    # the same seeds give the same ensemble, whatever torch's global generator has done in between
    torch.manual_seed(0); torch.rand(5)
    assert torch.equal(theta, init_ensemble_params(layers, "xavier", seeds))
    assert torch.equal(init_ensemble_params(layers, "kaiming", seeds)[2],
                       init_flat_params(layers, "kaiming", torch.Generator().manual_seed(13)))


def test_the_package_exports_the_trainer():
    import pinn_depthestimation_amd as P
    from pinn_depthestimation_amd.ensemble import EnsemblePINN
    assert P.EnsemblePINN is EnsemblePINN

"""Second-order jets (pinn_forward_jet2 / pinn_jet2_backward / pinn_query_jet2_workspace) without a GPU: the symbols
bind, every refusal comes back with its code and message before anything is launched, and the workspace query is
monotone in the point count (large requests run in point chunks, so it levels off)."""
import ctypes as C

import pytest

from pinn_depthestimation_amd import NetDesc, _lib
from pinn_depthestimation_amd._lib import ENGINE_FUSED, ENGINE_FUSED_COOP, ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
FAKE = C.c_void_p(0x1000)        # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def err(lib):
    return lib.pinn_last_error().decode()


def test_jet2_symbols_bind(lib):
    assert _lib.ABI_VERSION == 4 == lib.pinn_version()
    for name in ("pinn_forward_jet2", "pinn_jet2_backward", "pinn_query_jet2_workspace"):
        assert name in _lib.exported_symbols()
        assert getattr(lib, name).restype is C.c_int32


def test_jet2_validation_codes(lib):
    need = C.c_int64()
    d0 = NetDesc(3, 4, 8, 64, ()).c_struct()
    assert lib.pinn_query_jet2_workspace(C.byref(d0), 100, C.byref(need)) == INVALID and "k >= 1" in err(lib)
    assert lib.pinn_forward_jet2(C.byref(d0), FAKE, FAKE, 10, FAKE, FAKE, FAKE, FAKE, 1 << 20, None) == INVALID
    assert "k >= 1" in err(lib)
    assert lib.pinn_jet2_backward(C.byref(d0), FAKE, FAKE, 10, FAKE, None, None, FAKE, FAKE, 1 << 20, None) == INVALID
    good = NetDesc(3, 4, 8, 64, (0, 1, 2))
    for desc, what in ((good.with_(precision=PREC_BF16), "fp32 only"),
                       (good.with_(engine=ENGINE_WIDE), "wide engine"),
                       (good.with_(engine=ENGINE_FUSED, dropout_p=0.1), "dropout_p > 0"),
                       (good.with_(engine=ENGINE_FUSED_TILE, dropout_p=0.1), "dropout_p > 0"),
                       (NetDesc(3, 4, 8, 128, (0, 1, 2), engine=ENGINE_FUSED), "at most 64 wide"),
                       (NetDesc(3, 80, 8, 64, (0, 1, 2), engine=ENGINE_FUSED_COOP), "at most 64 wide")):
        c = desc.c_struct()
        assert lib.pinn_query_jet2_workspace(C.byref(c), 100, C.byref(need)) == UNSUPPORTED, what
        assert what in err(lib), (what, err(lib))
        assert lib.pinn_forward_jet2(C.byref(c), FAKE, FAKE, 10, FAKE, FAKE, FAKE, FAKE, 1 << 20, None) == UNSUPPORTED
        assert what in err(lib), (what, err(lib))
        assert lib.pinn_jet2_backward(C.byref(c), FAKE, FAKE, 10, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 20, None) == UNSUPPORTED
    # AUTO and GENERIC serve dropout (the generic kernels); FUSED serves the shapes its MFMA kernels cover
    for desc in (good.with_(dropout_p=0.1), good.with_(engine=ENGINE_GENERIC, dropout_p=0.1), good.with_(engine=ENGINE_FUSED),
                 NetDesc(2, 3, 100, 20, (0, 1), engine=ENGINE_FUSED_TILE), NetDesc(3, 4, 8, 128, (0, 1, 2))):
        assert lib.pinn_query_jet2_workspace(C.byref(desc.c_struct()), 100, C.byref(need)) == OK, err(lib)
    # shape / pointer / workspace errors of the usual kinds
    c = good.c_struct()
    assert lib.pinn_query_jet2_workspace(C.byref(c), -1, C.byref(need)) == INVALID
    assert lib.pinn_query_jet2_workspace(C.byref(c), 10, None) == INVALID
    assert lib.pinn_forward_jet2(C.byref(c), FAKE, FAKE, 10, FAKE, FAKE, None, FAKE, 1 << 20, None) == INVALID
    assert "NULL pointer" in err(lib)
    assert lib.pinn_forward_jet2(C.byref(c), None, FAKE, 10, FAKE, FAKE, FAKE, FAKE, 1 << 20, None) == INVALID
    assert lib.pinn_jet2_backward(C.byref(c), FAKE, FAKE, 10, FAKE, None, None, None, FAKE, 1 << 20, None) == INVALID
    assert lib.pinn_forward_jet2(C.byref(c), FAKE, FAKE, 10, FAKE, FAKE, FAKE, FAKE, 16, None) == WORKSPACE
    assert "workspace too small" in err(lib)
    assert lib.pinn_jet2_backward(C.byref(c), FAKE, FAKE, 10, FAKE, FAKE, FAKE, FAKE, FAKE, 16, None) == WORKSPACE
    assert lib.pinn_forward_jet2(C.byref(c), FAKE, None, 0, None, None, None, None, 0, None) == OK      # N = 0
    assert lib.pinn_jet2_backward(C.byref(c), FAKE, FAKE, 10, None, None, None, FAKE, None, 0, None) == OK  # nothing to add


@pytest.mark.parametrize("desc", [NetDesc(3, 4, 8, 64, (0, 1, 2)), NetDesc(2, 6, 10, 10, (0, 1)),
                                  NetDesc(2, 3, 100, 20, (0, 1)), NetDesc(3, 2, 2, 256, (1,))])
def test_jet2_workspace_monotone_and_bounded(lib, desc):
    need = C.c_int64()
    prev = 0
    sizes = []
    for N in (1, 15, 16, 17, 1000, 12514, 1 << 16, 1 << 20, 1 << 24):
        assert lib.pinn_query_jet2_workspace(C.byref(desc.c_struct()), N, C.byref(need)) == OK, err(lib)
        assert need.value >= prev, (N, need.value, prev)
        prev = need.value
        sizes.append(need.value)
    k = desc.k
    C_ch = 1 + k + k * (k + 1) // 2
    assert sizes[4] >= 1000 * 4 * C_ch * (2 * desc.n_hidden * desc.width)      # pre- and post-activation jets
    assert sizes[-1] == sizes[-2] and sizes[-1] <= (1 << 30) + (1 << 22)        # chunked: levels off near 1 GiB


def test_torch_engine_query_used_by_autograd_exists():
    """autograd.py decides whether a backward pass reaches the inputs with torch._C._will_engine_execute_node (checked
    against torch 2.10).  It is private API: if a torch upgrade removes it, this fails here, not inside a backward."""
    import torch
    assert callable(getattr(torch._C, "_will_engine_execute_node", None))
    x = torch.ones(3, requires_grad=True)
    y = x * 2
    seen = []
    z = y.view_as(y)

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a):
            return a.clone()

        @staticmethod
        def backward(ctx, g):
            seen.append(bool(torch._C._will_engine_execute_node(z.grad_fn)))
            return g

    w = Probe.apply(y)
    out = (w.sum() + z.sum())
    torch.autograd.grad(out, [x], retain_graph=True)       # z's node lies on the path to x
    torch.autograd.grad(w.sum(), [y], retain_graph=True)   # z's node is not needed for y
    assert seen == [True, False]

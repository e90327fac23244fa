"""pinn_jet_backward on the MFMA tile kernel, the parts that need no GPU: the Python signature, what the header says,
the ABI version, and the refusals the engine pick makes before anything touches a device."""
import ctypes as C
import inspect
import os

import pytest

from pinn_depthestimation_amd import Engine, NetDesc, _lib
from pinn_depthestimation_amd._lib import ENGINE_AUTO, ENGINE_FUSED, ENGINE_GENERIC, ENGINE_WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, WORKSPACE = 0, -2, -3


def test_engine_jet_backward_takes_an_engine_keyword():
    sig = inspect.signature(Engine.jet_backward)
    assert list(sig.parameters)[:6] == ["self", "params", "X", "gY", "gdY", "grad"]     # positional order is API
    assert "engine" in sig.parameters and sig.parameters["engine"].default is None


def test_header_states_the_engine_rules():
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert "always runs on the generic engine" not in text
    decl = text[:text.index("int32_t pinn_jet_backward(")]
    note = decl[decl.rindex("/*"):]
    for word in ("GENERIC", "FUSED", "WIDE", "AUTO", "PINN_ERR_UNSUPPORTED", "bit-reproducible"):
        assert word in note, word


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 4 and _lib.load().pinn_version() == 4


def _call(lib, desc, N=32, with_gdY=True):
    """pinn_jet_backward through the raw library with host buffers and NO workspace: a request that passes the engine
    pick stops at the workspace check, before any launch."""
    d = desc.c_struct()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    rc = lib.pinn_jet_backward(C.byref(d), p, p, N, p, p if with_gdY else None, p, None, 0, None)
    return rc, lib.pinn_last_error().decode()


def test_fused_refusals_are_decided_on_the_host():
    lib = _lib.load()
    rc, msg = _call(lib, NetDesc(3, 4, 2, 100, (0, 1, 2), engine=ENGINE_FUSED))
    assert rc == UNSUPPORTED and "width above 64" in msg, (rc, msg)
    rc, msg = _call(lib, NetDesc(3, 4, 2, 48, (1,), engine=ENGINE_FUSED))
    assert rc == UNSUPPORTED and "k = 1" in msg, (rc, msg)
    rc, msg = _call(lib, NetDesc(3, 4, 2, 48, (0, 1, 2), engine=ENGINE_FUSED, dropout_p=0.1))
    assert rc == UNSUPPORTED and "dropout" in msg, (rc, msg)
    rc, msg = _call(lib, NetDesc(3, 4, 2, 128, (0, 1, 2), engine=ENGINE_WIDE))
    assert rc == UNSUPPORTED and "wide engine" in msg, (rc, msg)
    # k = 1 WITHOUT gdY is the plain network (K1 = 1): served — the call gets as far as the workspace check
    rc, msg = _call(lib, NetDesc(3, 4, 2, 100, (0, 1, 2), engine=ENGINE_GENERIC))
    assert rc == WORKSPACE, (rc, msg)

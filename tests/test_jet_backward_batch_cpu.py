"""pinn_jet_backward_kernel, the host-side answer to "which kernel would pinn_jet_backward run": GENERIC, the fused tile
kernel or the fused batch kernel.  No GPU: the query is pure host logic and shares its decision with the call itself.
The AUTO / FUSED switch point is read from include/pinn_hip.h (PINN_JET_BACKWARD_BATCH_MIN_TILES), the place DESIGN.md
2.4b names."""
import ctypes as C
import os
import re

import pytest

from pinn_depthestimation_amd import Engine, NetDesc, PinnError, _lib
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
OK, UNSUPPORTED = 0, -2
GENERIC, TILE, BATCH = ENGINE_GENERIC, ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH
FUSED_ALL = (ENGINE_FUSED, ENGINE_FUSED_TILE, ENGINE_FUSED_COOP, ENGINE_FUSED_BATCH)
BIG = 1 << 20


def threshold_tiles():
    m = re.search(r"#define\s+PINN_JET_BACKWARD_BATCH_MIN_TILES\s+(\d+)", HEADER)
    assert m, "pinn_hip.h must define PINN_JET_BACKWARD_BATCH_MIN_TILES"
    return int(m.group(1))


def query(desc, N, with_gdY=True):
    """(return code, kernel, message) of the raw C entry."""
    lib = _lib.load()
    d = desc.c_struct()
    kern = C.c_int32(-99)
    rc = lib.pinn_jet_backward_kernel(C.byref(d), N, 1 if with_gdY else 0, C.byref(kern))
    return rc, kern.value, lib.pinn_last_error().decode()


def kernel_of(desc, N, with_gdY=True):
    rc, kern, msg = query(desc, N, with_gdY)
    assert rc == OK, (rc, msg)
    return kern


PE10 = NetDesc(2, 6, 10, 10, (0, 1))


def test_the_design_document_names_the_same_threshold():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "PINN_JET_BACKWARD_BATCH_MIN_TILES" in design
    assert f"PINN_JET_BACKWARD_BATCH_MIN_TILES = {threshold_tiles()}" in design


@pytest.mark.parametrize("engine", [ENGINE_AUTO, ENGINE_FUSED])
def test_auto_and_fused_switch_at_the_threshold(engine):
    thr = threshold_tiles()
    d = PE10.with_(engine=engine)
    assert kernel_of(d, 16 * thr - 1) == TILE
    assert kernel_of(d, 16 * thr) == BATCH
    assert kernel_of(d, BIG) == BATCH


def test_fused_batch_forces_the_batch_kernel_at_any_size():
    assert kernel_of(PE10.with_(engine=ENGINE_FUSED_BATCH), 1) == BATCH


@pytest.mark.parametrize("engine", [ENGINE_FUSED_TILE, ENGINE_FUSED_COOP])
def test_tile_and_coop_keep_the_tile_kernel(engine):
    assert kernel_of(PE10.with_(engine=engine), BIG) == TILE


NO_BATCH_INSTANCE = {
    "leaky_relu": (NetDesc(2, 6, 10, 10, (0, 1), ACT_LEAKY_RELU), True),
    "d_in_9": (NetDesc(9, 4, 3, 20, (0, 1, 2)), True),
    "width_33": (NetDesc(2, 6, 4, 33, (0, 1)), True),
    "k_0": (NetDesc(2, 6, 10, 10, ()), True),
    "k_1_without_gdY": (NetDesc(2, 6, 10, 10, (1,)), False),
}


@pytest.mark.parametrize("engine", [ENGINE_FUSED_BATCH, ENGINE_AUTO])
@pytest.mark.parametrize("name", sorted(NO_BATCH_INSTANCE))
def test_requests_without_a_batch_instance_stay_on_the_tile_kernel(name, engine):
    desc, with_gdY = NO_BATCH_INSTANCE[name]
    assert kernel_of(desc.with_(engine=engine), BIG, with_gdY) == TILE


NOT_ON_FUSED = {
    "width_100": (NetDesc(3, 4, 2, 100, (0, 1, 2)), "width"),
    "dropout": (NetDesc(2, 3, 3, 20, (0, 1), dropout_p=0.25), "dropout"),
    "k1_with_gdY": (NetDesc(3, 4, 3, 20, (1,)), "k = 1"),
}


@pytest.mark.parametrize("name", sorted(NOT_ON_FUSED))
def test_auto_sends_them_to_the_generic_engine_and_fused_refuses(name):
    desc, why = NOT_ON_FUSED[name]
    assert kernel_of(desc.with_(engine=ENGINE_AUTO), BIG) == GENERIC
    assert kernel_of(desc.with_(engine=ENGINE_GENERIC), BIG) == GENERIC
    for engine in FUSED_ALL:
        rc, kern, msg = query(desc.with_(engine=engine), BIG)
        assert rc == UNSUPPORTED and why in msg, (engine, rc, msg)
        assert kern == -99                       # nothing is written on a refusal


def test_the_query_refuses_with_the_calls_own_message():
    """The same descriptor through pinn_jet_backward itself (host buffers, no workspace: refused before any launch)."""
    lib = _lib.load()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    for name, (desc, why) in NOT_ON_FUSED.items():
        d = desc.with_(engine=ENGINE_FUSED_BATCH).c_struct()
        rc = lib.pinn_jet_backward(C.byref(d), p, p, 32, p, p, p, None, 0, None)
        msg_call = lib.pinn_last_error().decode()
        rc_q, _, msg_q = query(desc.with_(engine=ENGINE_FUSED_BATCH), 32)
        assert rc == rc_q == UNSUPPORTED and msg_call == msg_q, (name, msg_call, msg_q)


def test_wide_is_refused():
    rc, _, msg = query(NetDesc(3, 4, 3, 128, (0, 1, 2), engine=ENGINE_WIDE), BIG)
    assert rc == UNSUPPORTED and "wide engine" in msg, (rc, msg)
    rc, _, msg = query(PE10.with_(engine=ENGINE_WIDE), BIG)
    assert rc == UNSUPPORTED and "wide engine" in msg, (rc, msg)


def test_bad_arguments():
    lib = _lib.load()
    d = PE10.c_struct()
    assert lib.pinn_jet_backward_kernel(C.byref(d), 16, 1, None) == -1
    kern = C.c_int32()
    assert lib.pinn_jet_backward_kernel(C.byref(d), -1, 1, C.byref(kern)) == -1


def test_engine_method_answers_as_the_library_does():
    eng = Engine(PE10, "cuda")              # (binds no device until a call that needs one)
    thr = threshold_tiles()
    assert eng.jet_backward_kernel(16 * thr - 1) == TILE and eng.jet_backward_kernel(16 * thr) == BATCH
    assert eng.jet_backward_kernel(1, engine=ENGINE_FUSED_BATCH) == BATCH
    assert eng.jet_backward_kernel(BIG, engine=ENGINE_FUSED_TILE) == TILE
    assert eng.jet_backward_kernel(BIG, with_gdY=False) == TILE
    assert eng.jet_backward_kernel(BIG, engine=ENGINE_GENERIC) == GENERIC
    with pytest.raises(PinnError, match="wide engine"):
        eng.jet_backward_kernel(BIG, engine=ENGINE_WIDE)


def test_header_and_library_export_the_same_set_and_the_abi_version_stays():
    declared = set(re.findall(r"\b(pinn_[a-z0-9_]+)\s*\(", HEADER))
    bound = set(_lib.exported_symbols())
    assert "pinn_jet_backward_kernel" in declared and "pinn_jet_backward_kernel" in bound
    assert declared == bound, (sorted(declared - bound), sorted(bound - declared))
    lib = _lib.load()
    for name in declared:
        getattr(lib, name)
    assert _lib.ABI_VERSION == 4 and lib.pinn_version() == 4
    assert re.search(r"#define\s+PINN_ABI_VERSION\s+4\b", HEADER)

"""pinn_jet_backward on the fused BATCH kernel (k_fused_batch with the external-adjoint epilogue): user-written PDE
residuals on narrow tanh networks.  Checkers: oracle/pinn_oracle.py in float64 for the one-tile instances, the GENERIC
engine (oracle-pinned, reproducible) for the full-batch instances.  Gradient bar: the project's rel_l2 < 2e-5
(tests/test_jet_backward_mfma_gpu.py, whose helpers are copied here).  Every case first asks
Engine.jet_backward_kernel which kernel will run, so a silent fallback to the tile kernel cannot pass as the feature."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, _lib
from pinn_depthestimation_amd._lib import (ENGINE_AUTO, ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE, ENGINE_GENERIC)

pytestmark = pytest.mark.gpu

TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def threshold_tiles():
    text = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    return int(re.search(r"#define\s+PINN_JET_BACKWARD_BATCH_MIN_TILES\s+(\d+)", text).group(1))


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def make(desc, N, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(desc.layers, "xavier", g)
    X = torch.rand(N, desc.d_in, generator=g) * 2 - 1
    gY = torch.randn(N, desc.d_out, generator=g) * scale
    gdY = torch.randn(desc.k, N, desc.d_out, generator=g) * scale
    return params, X, gY, gdY


def oracle_grad(desc, params, X, gY, gdY):
    """float64 d/dtheta [sum(gY * Y) + sum(gdY * dY)] by torch autograd over the oracle's network."""
    p64 = [p.double().clone().requires_grad_(True) for p in params]
    cols = O.split_columns(X.double(), desc.grad_cols)
    Y = O.mlp_forward(p64, torch.cat(cols, -1), "xavier")
    obj = 0.0
    if gY is not None:
        obj = obj + (gY.double() * Y).sum()
    if gdY is not None:
        dY = torch.stack([torch.cat([O.compute_gradient(Y[:, c:c + 1], cols[j]) for c in range(desc.d_out)], 1)
                          for j in desc.grad_cols])
        obj = obj + (gdY.double() * dY).sum()
    return O.flat_grad(obj, p64)


def dev(t):
    return None if t is None else t.cuda()


def run(desc, engine, params, X, gY, gdY, grad=None, eng=None):
    eng = Engine(desc.with_(engine=engine)) if eng is None else eng
    grad = torch.zeros(desc.n_params, device="cuda") if grad is None else grad
    eng.jet_backward(O.flatten(params).cuda(), dev(X), dev(gY), dev(gdY), grad)
    torch.cuda.synchronize()
    return grad


def assert_batch(desc, N, engine=ENGINE_FUSED_BATCH):
    assert Engine(desc.with_(engine=engine)).jet_backward_kernel(N) == ENGINE_FUSED_BATCH, (desc, N)


PE10 = NetDesc(2, 6, 10, 10, (0, 1))            # KS 3, gradient copies in LDS
A40 = NetDesc(2, 3, 40, 20, (0, 1))             # KS 5, atomic sink

# ---- 1. every instance family at T = 1 against the fp64 oracle ----------------------------------------------------------
CASES = {
    "ks3_lds_10x10": (PE10, 700),
    "ks4_3x16_k3": (NetDesc(3, 4, 3, 16, (0, 1, 2)), 333),
    "ks5_4x20_k3": (NetDesc(4, 4, 4, 20, (0, 1, 2)), 333),
    "ks8_3x32": (NetDesc(2, 3, 3, 32, (0, 1)), 200),
    "ks0_2_din8": (NetDesc(8, 5, 2, 20, (1, 4, 7)), 150),
    "dout16_2x12": (NetDesc(3, 16, 2, 12, (0, 1)), 97),
    "single_hidden_1x10": (NetDesc(2, 6, 1, 10, (0, 1)), 333),
    "atomic_40x20": (A40, 333),
    "atomic_40x20_k3": (NetDesc(3, 3, 40, 20, (0, 1, 2)), 120),
    "n_1": (PE10, 1),
    "n_15": (PE10, 15),
    "n_16": (PE10, 16),
    "n_17": (PE10, 17),
    "n_17_atomic": (A40, 17),
    "wg_trip_lds": (PE10, 16 * 4 + 1),           # waves past the end must contribute exact zeros ...
    "wg_trip_atomic": (A40, 16 * 4 + 1),         # ... also at the __syncthreads of the workgroup flush
}


@pytest.mark.parametrize("mode", ["both", "gY", "gdY"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_tile_instances_against_the_fp64_oracle(name, mode):
    desc, N = CASES[name]
    assert_batch(desc, N)
    params, X, gY, gdY = make(desc, N, seed=43)
    gY = None if mode == "gdY" else gY
    gdY = None if mode == "gY" else gdY
    ref = oracle_grad(desc, params, X, gY, gdY)
    if gdY is None:
        # gdY == NULL is the plain network (k = 0), which has no batch instance: FUSED_BATCH serves it on the tile kernel ...
        assert Engine(desc.with_(engine=ENGINE_FUSED_BATCH)).jet_backward_kernel(N, with_gdY=False) == ENGINE_FUSED_TILE
        rel = rel_l2(run(desc, ENGINE_FUSED_BATCH, params, X, gY, None), ref)
        assert rel < TOL, (name, mode, "tile kernel", rel)
        gdY = torch.zeros(desc.k, N, desc.d_out)       # ... and the batch kernel gets the same request with zero tangent adjoints
    got = run(desc, ENGINE_FUSED_BATCH, params, X, gY, gdY)
    rel = rel_l2(got, ref)
    print(f"{name} {mode}: rel_l2 {rel:.2e}")
    assert rel < TOL, (name, mode, rel)


# ---- 2. full-batch instances (T = batch_tiles) against the GENERIC engine ------------------------------------------------
FULL = {
    "lds_10x10": PE10,
    "3x16_k3": NetDesc(3, 4, 3, 16, (0, 1, 2)),
    "4x20_k3": NetDesc(4, 4, 4, 20, (0, 1, 2)),
    "atomic_40x20": A40,
}


def full_batch_n(desc):
    """The size from which every wave of the chip gets a full batch of tiles for both K1 (batch_T_for, pinn_fused.hip:
    CUs x 4 waves x waves per SIMD x tiles per batch x 16 points = CUs x 512 at padded width 16, CUs x 256 at 32);
    + 53 makes the last batch and the last tile ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * 4 * 16 * (8 if desc.width <= 16 else 4) + 53


@functools.lru_cache(maxsize=None)
def full_batch_runs(name):
    """(generic, four FUSED_BATCH runs) of one full-batch case: computed once, shared by the tests below, never changed."""
    desc = FULL[name]
    N = full_batch_n(desc)
    assert_batch(desc, N)
    params, X, gY, gdY = make(desc, N, seed=47, scale=1.0 / N)
    generic = run(desc, ENGINE_GENERIC, params, X, gY, gdY)
    eng = Engine(desc.with_(engine=ENGINE_FUSED_BATCH))
    return generic, [run(desc, ENGINE_FUSED_BATCH, params, X, gY, gdY, eng=eng) for _ in range(4)]


@pytest.mark.parametrize("name", sorted(FULL))
def test_full_batch_instances_against_the_generic_engine(name):
    generic, runs = full_batch_runs(name)
    rel = rel_l2(runs[0], generic)
    print(f"{name} N={full_batch_n(FULL[name])}: batch vs generic {rel:.2e}")
    assert bool(torch.isfinite(runs[0]).all()) and rel < TOL, (name, rel)


# ---- 3. reproducibility -------------------------------------------------------------------------------------------------
def test_lds_sink_is_bit_reproducible_at_every_size():
    """A gradient copy per wave, program order, fixed-order sums (include/pinn_hip.h).  The tile kernel does not promise
    this at the larger size (N > 16 x its workgroups)."""
    params, X, gY, gdY = make(PE10, 700, seed=12)
    assert_batch(PE10, 700)
    first = run(PE10, ENGINE_FUSED_BATCH, params, X, gY, gdY)
    for _ in range(3):
        assert torch.equal(run(PE10, ENGINE_FUSED_BATCH, params, X, gY, gdY), first)
    _, runs = full_batch_runs("lds_10x10")
    for r in runs[1:]:
        assert torch.equal(r, runs[0])


def test_atomic_sink_repeats_within_the_run_to_run_bar():
    params, X, gY, gdY = make(A40, 333, seed=12)
    first = run(A40, ENGINE_FUSED_BATCH, params, X, gY, gdY)
    for _ in range(3):
        assert rel_l2(run(A40, ENGINE_FUSED_BATCH, params, X, gY, gdY), first) < 1e-6
    _, runs = full_batch_runs("atomic_40x20")
    for r in runs[1:]:
        assert rel_l2(r, runs[0]) < 1e-6


# ---- 4. buffer contract: +=, dirty workspace, guard band ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ks3_lds_10x10", "atomic_40x20"])
def test_buffer_contract(name):
    desc, _ = CASES[name]
    N = 333
    lds_sink = name == "ks3_lds_10x10"
    assert_batch(desc, N)
    params, X, gY, gdY = make(desc, N, seed=5)
    eng = Engine(desc.with_(engine=ENGINE_FUSED_BATCH))
    g0 = run(desc, ENGINE_FUSED_BATCH, params, X, gY, gdY, eng=eng)
    assert rel_l2(g0, oracle_grad(desc, params, X, gY, gdY)) < TOL
    # += into what grad holds, with a 64-float guard band behind it
    P = desc.n_params
    pre = torch.randn(P, generator=torch.Generator().manual_seed(6)).cuda()
    buf = torch.full((P + 64,), 12345.678, device="cuda")
    buf[:P] = pre
    g1 = run(desc, ENGINE_FUSED_BATCH, params, X, gY, gdY, grad=buf[:P], eng=eng)
    assert rel_l2(g1 - pre, g0) < 1e-6
    assert float((g1 - pre).abs().max()) > 0.0
    assert bool((buf[P:] == 12345.678).all())
    # every byte of the workspace holds a NaN pattern before the call
    ws = eng.workspace(N)
    ws.view(torch.int32)[:ws.numel() // 4].fill_(0x7FC00000)
    g2 = run(desc, ENGINE_FUSED_BATCH, params, X, gY, gdY, eng=eng)
    assert eng.workspace(N).data_ptr() == ws.data_ptr()
    assert bool(torch.isfinite(g2).all())
    if lds_sink:
        assert torch.equal(g2, g0)
    else:
        assert rel_l2(g2, g0) < 1e-6


# ---- 5. history on ONE engine and ONE workspace ---------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("name", ["ks3_lds_10x10", "atomic_40x20"])
def test_kernels_take_turns_on_one_workspace(name):
    """Each kernel packs the weights in its own unit order and carves the spill area its own way: a call must not depend
    on what the previous one left behind.  Raw C calls, so that every engine value gets the SAME workspace bytes."""
    desc, N = CASES[name]
    params, X, gY, gdY = make(desc, N, seed=9)
    flat, Xd, gYd, gdYd = O.flatten(params).cuda(), X.cuda(), gY.cuda(), gdY.cuda()
    lib = _lib.load()
    eng = Engine(desc)
    ws = torch.empty(max(eng.workspace(N, e).numel() for e in (ENGINE_AUTO, ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH)),
                     dtype=torch.uint8, device="cuda")

    def jet_backward(engine):
        grad = torch.zeros(desc.n_params, device="cuda")
        d = desc.with_(engine=engine).c_struct()
        _lib.check(lib.pinn_jet_backward(C.byref(d), _p(flat), _p(Xd), N, _p(gYd), _p(gdYd), _p(grad), _p(ws), ws.numel(),
                                         _stream()), "pinn_jet_backward")
        torch.cuda.synchronize()
        return grad

    names = ("U", "V", "h") if desc.d_out == 3 else ("h", "U", "V", "eta_mean", "Hrms", "k")
    spec = ResidualSpec.from_names("continuity_ftemp", ("x", "y"), desc.grad_cols, names)

    def residual_loss_grad(engine):
        grad = torch.zeros(desc.n_params, device="cuda")
        scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
        sums = torch.empty(spec.n_terms, device="cuda")
        d = desc.with_(engine=engine).c_struct()
        _lib.check(lib.pinn_residual_loss_grad(C.byref(d), C.byref(spec.c_struct()), _p(scale), _p(flat), _p(Xd), N, _p(sums),
                                               _p(grad), _p(ws), ws.numel(), _stream()), "pinn_residual_loss_grad")
        torch.cuda.synchronize()
        return grad

    fresh = {e: run(desc, e, params, X, gY, gdY) for e in (ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH)}
    assert Engine(desc.with_(engine=ENGINE_FUSED_BATCH)).jet_backward_kernel(N) == ENGINE_FUSED_BATCH
    assert Engine(desc.with_(engine=ENGINE_FUSED_TILE)).jet_backward_kernel(N) == ENGINE_FUSED_TILE
    for e in (ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE):
        rel = rel_l2(jet_backward(e), fresh[e])
        assert rel < TOL, (name, e, rel)
    loss_grad = residual_loss_grad(ENGINE_FUSED_BATCH)
    assert bool(torch.isfinite(loss_grad).all())
    rel = rel_l2(jet_backward(ENGINE_FUSED_BATCH), fresh[ENGINE_FUSED_BATCH])
    assert rel < TOL, (name, "after residual_loss_grad", rel)


# ---- 6. the drop-in face --------------------------------------------------------------------------------------------------
def burgers(t, x, y, h, z, u, v):
    from pinn_depthestimation_amd.physics import compute_gradient as d
    r1 = d(u, t) + u * d(u, x) + v * d(u, y)
    r2 = d(v, t) + u * d(v, x) + v * d(v, y) + 0.3 * d(h + z, y)
    return torch.mean(r1 ** 2) + torch.mean(r2 ** 2) + 0.1 * torch.mean((h - 0.5) ** 2)


def corrected_pe(x, y, *outs):
    from pinn_depthestimation_amd import physics
    return physics.physics_equation(x, y, *outs, corrected=True)


def dropin_model(layers, seed):
    from pinn_depthestimation_amd.dnn import DNN
    torch.manual_seed(seed)
    model = DNN(layers, 0.0, "xavier").to("cuda")
    if layers[-1] == 6:       # keep eta_mean + h away from 0 and k h away from 0 (1 / sinh(2 k h))
        last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.bias[4] = 0.2; last.bias[5] = 1.0; last.bias[0] = 2.0
    return model


def fp64_reference(model, Xh, loss_fn):
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in model._ordered_params()]
    cols = [Xh[:, i:i + 1].double().clone().requires_grad_(True) for i in range(Xh.shape[1])]
    pred = O.mlp_forward(p64, torch.cat(cols, -1))
    loss = loss_fn(*cols, *[pred[:, i:i + 1] for i in range(pred.shape[1])])
    return loss, O.flat_grad(loss, p64)


@pytest.mark.parametrize("case", ["burgers_4x20", "corrected_pe_10x10"])
def test_custom_residual_through_the_drop_in_face_takes_the_batch_kernel(case, monkeypatch):
    layers, loss_fn = {"burgers_4x20": ([3, 20, 20, 20, 20, 4], burgers),
                       "corrected_pe_10x10": ([2] + [10] * 10 + [6], corrected_pe)}[case]
    N = 16 * threshold_tiles() + 37
    seen = []
    orig = Engine.jet_backward

    def spy(self, params, X, gY, gdY, grad, engine=None):
        seen.append((self.desc.engine, engine, gdY is not None, self.jet_backward_kernel(X.shape[0], gdY is not None, engine)))
        return orig(self, params, X, gY, gdY, grad, engine)

    monkeypatch.setattr(Engine, "jet_backward", spy)
    model = dropin_model(layers, seed=3)
    Xh = torch.rand(N, layers[0], generator=torch.Generator().manual_seed(5)) * 2 - 1
    cols = [Xh[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(layers[0])]
    pred = model(torch.cat(cols, -1))
    loss = loss_fn(*cols, *[pred[:, i:i + 1] for i in range(layers[-1])])
    model.zero_grad()
    loss.backward()
    got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
    lo, go = fp64_reference(model, Xh, loss_fn)
    lo = lo.detach()
    rel = rel_l2(got, go)
    print(f"{case}: loss {loss.item():.6e} (fp64 {float(lo):.6e}) grad rel_l2 {rel:.2e}; jet_backward calls {seen}")
    assert abs(loss.item() - float(lo)) / abs(float(lo)) < 5e-6
    assert rel < TOL
    # the reverse sweeps ran on the descriptor's own engine, AUTO, with no override — and AUTO took the batch kernel for
    # the sweep that carries the tangents' adjoints (the plain network's sweep, gdY = None, has k = 0: the tile kernel)
    assert 1 <= len(seen) <= 2 and all(s[:2] == (ENGINE_AUTO, None) for s in seen), seen
    jets = [s for s in seen if s[2]]
    assert jets and all(s[3] == ENGINE_FUSED_BATCH for s in jets), seen
    assert all(s[3] == ENGINE_FUSED_TILE for s in seen if not s[2]), seen

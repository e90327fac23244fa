"""Second-order input derivatives on the GPU: Engine.forward_jet2 / jet2_backward against fp64 torch double-backward
through oracle.mlp_forward, and the drop-in face (nested physics.compute_gradient on a DNN) against an fp64 copy.

Tolerances: Y / dY as the first-order tests (rel_l2 < 2e-5); d2Y and every parameter gradient rel_l2 <= 1e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, PinnError, _lib
from pinn_depthestimation_amd._lib import ACT_LEAKY_RELU, ACT_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_GENERIC
from tests.dropout_util import keep_masks

pytestmark = pytest.mark.gpu

TOL1, TOL2 = 2e-5, 1e-4


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def pairs(k):
    return [(i, j) for i in range(k) for j in range(i, k)]


def ref_jets(params, X, grad_cols, init_type="xavier", masks=None, p=0.0, device="cpu"):
    """fp64 (params, Y, dY, d2Y) by nested torch.autograd.grad (physics.py:6-15 applied twice)."""
    p64 = [q.detach().double().to(device).requires_grad_(True) for q in params]
    cols = [X[:, i:i + 1].detach().double().to(device).requires_grad_(True) for i in range(X.shape[1])]
    if masks is not None:
        masks = [m.to(device) for m in masks]
    Y = O.mlp_forward(p64, torch.cat(cols, -1), init_type, masks, p)

    def g(a, b):
        r = torch.autograd.grad(a.sum(), b, create_graph=True, allow_unused=True)[0]
        return torch.zeros_like(b) if r is None else r

    d_out = Y.shape[1]
    dY = torch.stack([torch.cat([g(Y[:, c:c + 1], cols[j]) for c in range(d_out)], 1) for j in grad_cols])
    d2Y = torch.stack([torch.cat([g(dY[i][:, c:c + 1], cols[grad_cols[j]]) for c in range(d_out)], 1)
                       for i, j in pairs(len(grad_cols))])
    return p64, Y, dY, d2Y


def ref_grad(p64, Y, dY, d2Y, gY, gdY, gd2Y):
    L = 0
    for adj, val in ((gY, Y), (gdY, dY), (gd2Y, d2Y)):
        if adj is not None:
            L = L + (adj.double().to(val.device) * val).sum()
    gs = torch.autograd.grad(L, p64, allow_unused=True, retain_graph=True)     # (the jets serve several adjoints)
    return torch.cat([(g if g is not None else torch.zeros_like(p)).reshape(-1) for g, p in zip(gs, p64)])


def setup(desc, N, seed=0, init_type="xavier"):
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(desc.layers, init_type, g)
    X = torch.rand(N, desc.d_in, generator=g) * 2 - 1
    return params, X


SHAPES = [
    ("8x64_k3", NetDesc(3, 4, 8, 64, (0, 1, 2)), 600),
    ("10x10_k2", NetDesc(2, 6, 10, 10, (0, 1)), 700),
    ("100x20_k2", NetDesc(2, 3, 100, 20, (0, 1)), 300),
    ("w17_k2", NetDesc(3, 2, 3, 17, (2, 0)), 333),
    ("leaky_4x32_k3", NetDesc(3, 3, 4, 32, (0, 1, 2), activation=ACT_LEAKY_RELU), 500),
    ("w256_k2", NetDesc(3, 4, 3, 256, (1, 2)), 250),
    ("N_odd_k1", NetDesc(3, 2, 4, 24, (1,)), 37),
]


@pytest.mark.parametrize("name,desc,N", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("engine", [ENGINE_GENERIC, ENGINE_FUSED, ENGINE_AUTO])
def test_forward_jet2_and_backward_against_fp64(name, desc, N, engine):
    init = "kaiming" if desc.activation == ACT_LEAKY_RELU else "xavier"
    params, X = setup(desc, N, init_type=init)
    eng = Engine(desc.with_(engine=engine), "cuda")
    flat, Xc = O.flatten(params).cuda(), X.cuda()
    if engine == ENGINE_FUSED and desc.width > 64:        # the MFMA kernels stop at 64; AUTO takes the generic ones
        with pytest.raises(PinnError, match="at most 64 wide"):
            eng.forward_jet2(flat, Xc)
        return
    p64, Y, dY, d2Y = ref_jets(params, X, desc.grad_cols, init)
    gotY, got_dY, got_d2Y = eng.forward_jet2(flat, Xc)
    assert got_d2Y.shape == (desc.k * (desc.k + 1) // 2, N, desc.d_out)
    assert rel_l2(gotY, Y) < TOL1 and rel_l2(got_dY, dY) < TOL1
    assert rel_l2(got_d2Y, d2Y) < TOL2, rel_l2(got_d2Y, d2Y)
    # first order agrees with the first-order kernels
    Y1, dY1 = Engine(desc.with_(engine=ENGINE_GENERIC), "cuda").forward_jet(flat, Xc)
    assert rel_l2(gotY, Y1) < TOL1 and rel_l2(got_dY, dY1) < TOL1
    g = torch.Generator().manual_seed(7)
    gY = torch.randn(N, desc.d_out, generator=g)
    gdY = torch.randn(desc.k, N, desc.d_out, generator=g)
    gd2Y = torch.randn(*got_d2Y.shape, generator=g)
    for adj in ((gY, gdY, gd2Y), (gY, None, None), (None, gdY, None), (None, None, gd2Y)):
        grad = torch.zeros_like(flat)
        eng.jet2_backward(flat, Xc, *[a.cuda() if a is not None else None for a in adj], grad)
        ref = ref_grad(p64, Y, dY, d2Y, *adj)
        assert rel_l2(grad, ref) < TOL2, ([a is not None for a in adj], rel_l2(grad, ref))


def test_fused_engine_refusals_for_jet2():
    params, X = setup(NetDesc(3, 4, 8, 64, (0, 1, 2)), 64)
    with pytest.raises(PinnError, match="dropout_p > 0"):
        Engine(NetDesc(3, 4, 8, 64, (0, 1, 2), engine=ENGINE_FUSED, dropout_p=0.1), "cuda").forward_jet2(
            O.flatten(params).cuda(), X.cuda())


def test_mfma_and_generic_agree():
    """The MFMA kernels (FUSED) against the generic kernels, the on-device check: same jets and gradients to fp32
    rounding (different summation order), on the headline shape with N not a multiple of 16."""
    desc = NetDesc(3, 4, 8, 64, (0, 1, 2))
    N = 4099
    params, X = setup(desc, N, seed=21)
    flat, Xc = O.flatten(params).cuda(), X.cuda()
    g = torch.Generator().manual_seed(4)
    adj = [torch.randn(N, 4, generator=g).cuda(), torch.randn(3, N, 4, generator=g).cuda(),
           torch.randn(6, N, 4, generator=g).cuda()]
    out = {}
    for e in (ENGINE_FUSED, ENGINE_GENERIC):
        eng = Engine(desc.with_(engine=e), "cuda")
        grad = torch.zeros_like(flat)
        out[e] = (*eng.forward_jet2(flat, Xc), eng.jet2_backward(flat, Xc, *adj, grad))
    for a, b in zip(out[ENGINE_FUSED], out[ENGINE_GENERIC]):
        assert rel_l2(a, b) < 2e-6, rel_l2(a, b)


def test_jet2_dropout_generic_against_fp64_with_engine_mask():
    desc = NetDesc(3, 4, 4, 40, (0, 1, 2), dropout_p=0.1)
    N, seed = 400, 12345
    params, X = setup(desc, N, seed=3)
    masks = [torch.from_numpy(m).double() for m in keep_masks(seed, 0.1, desc.n_hidden, desc.width, N)]
    p64, Y, dY, d2Y = ref_jets(params, X, desc.grad_cols, "xavier", masks, 0.1)
    eng = Engine(desc.with_(engine=ENGINE_GENERIC), "cuda")
    eng.dropout_seed = seed
    flat, Xc = O.flatten(params).cuda(), X.cuda()
    gotY, got_dY, got_d2Y = eng.forward_jet2(flat, Xc)
    assert rel_l2(gotY, Y) < TOL1 and rel_l2(got_dY, dY) < TOL1 and rel_l2(got_d2Y, d2Y) < TOL2
    g = torch.Generator().manual_seed(1)
    adj = (torch.randn(N, 4, generator=g), torch.randn(3, N, 4, generator=g), torch.randn(6, N, 4, generator=g))
    grad = torch.zeros_like(flat)
    eng.jet2_backward(flat, Xc, *[a.cuda() for a in adj], grad)
    assert rel_l2(grad, ref_grad(p64, Y, dY, d2Y, *adj)) < TOL2


def chunk_points(desc):
    """Points per chunk of a jet2 call: the smallest N whose workspace is the (levelled-off) largest one."""
    lib, need = _lib.load(), C.c_int64()
    c = desc.c_struct()

    def ws(n):
        assert lib.pinn_query_jet2_workspace(C.byref(c), n, C.byref(need)) == 0
        return need.value

    top, lo, hi = ws(1 << 40), 1, 1 << 40
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ws(mid) >= top else (mid + 1, hi)
    return lo


@pytest.mark.parametrize("engine", [ENGINE_FUSED, ENGINE_GENERIC])
def test_jet2_multi_chunk_against_fp64_and_per_chunk_calls(engine):
    """A request of 2 chunks + 77 points: forward and backward against fp64, head / tail rows against separate calls,
    and the backward against the sum of per-chunk calls."""
    desc = NetDesc(3, 4, 8, 64, (0, 1, 2), engine=engine)
    Nc = chunk_points(desc)
    N = 2 * Nc + 77
    params, X = setup(desc, N, seed=8)
    eng = Engine(desc, "cuda")
    flat, Xc = O.flatten(params).cuda(), X.cuda()
    Y, dY, d2Y = eng.forward_jet2(flat, Xc)
    p64, Yr, dYr, d2Yr = ref_jets(params, X, desc.grad_cols, device="cuda")
    assert rel_l2(Y, Yr) < TOL1 and rel_l2(dY, dYr) < TOL1 and rel_l2(d2Y, d2Yr) < TOL2
    g = torch.Generator().manual_seed(6)
    adj = [torch.randn(N, 4, generator=g).cuda(), torch.randn(3, N, 4, generator=g).cuda(),
           torch.randn(6, N, 4, generator=g).cuda()]
    grad = eng.jet2_backward(flat, Xc, *adj, torch.zeros_like(flat))
    assert rel_l2(grad, ref_grad(p64, Yr, dYr, d2Yr, *adj)) < TOL2
    for sl in (slice(0, 300), slice(N - 300, N)):
        _, dYs, d2Ys = eng.forward_jet2(flat, Xc[sl].contiguous())
        assert torch.equal(dY[:, sl], dYs) and torch.equal(d2Y[:, sl], d2Ys)
    parts = torch.zeros_like(flat)
    for a in range(0, N, Nc):
        sl = slice(a, min(a + Nc, N))
        eng.jet2_backward(flat, Xc[sl].contiguous(), adj[0][sl].contiguous(), adj[1][:, sl].contiguous(),
                          adj[2][:, sl].contiguous(), parts)
    assert rel_l2(grad, parts) < 1e-6


def test_jet2_multi_chunk_dropout_against_fp64():
    """Dropout's mask is a function of the GLOBAL point index: a multi-chunk request against fp64 fed that mask."""
    desc = NetDesc(3, 4, 6, 256, (0, 2), dropout_p=0.1)
    Nc = chunk_points(desc)
    N, seed = Nc + 301, 777
    params, X = setup(desc, N, seed=9)
    masks = [torch.from_numpy(m).double() for m in keep_masks(seed, 0.1, desc.n_hidden, desc.width, N)]
    eng = Engine(desc, "cuda")
    eng.dropout_seed = seed
    flat, Xc = O.flatten(params).cuda(), X.cuda()
    Y, dY, d2Y = eng.forward_jet2(flat, Xc)
    p64, Yr, dYr, d2Yr = ref_jets(params, X, desc.grad_cols, "xavier", masks, 0.1, device="cuda")
    assert rel_l2(Y, Yr) < TOL1 and rel_l2(dY, dYr) < TOL1 and rel_l2(d2Y, d2Yr) < TOL2
    g = torch.Generator().manual_seed(2)
    adj = [torch.randn(N, 4, generator=g).cuda(), torch.randn(2, N, 4, generator=g).cuda(),
           torch.randn(3, N, 4, generator=g).cuda()]
    grad = eng.jet2_backward(flat, Xc, *adj, torch.zeros_like(flat))
    assert rel_l2(grad, ref_grad(p64, Yr, dYr, d2Yr, *adj)) < TOL2


# ---- the drop-in face: nested compute_gradient --------------------------------------------------------------------


NU = 0.05


def _heat_residual_ref(sd_params, cols):
    t, x, y = cols
    u = O.mlp_forward(sd_params, torch.cat(cols, -1))[:, 0:1]
    d = O.compute_gradient
    u_x, u_y = d(u, x), d(u, y)
    return ((d(u, t) - NU * (d(u_x, x) + d(u_y, y))) ** 2).mean()


def _model(seed=11):
    from pinn_depthestimation_amd.dnn import DNN
    torch.manual_seed(seed)
    return DNN([3, 32, 32, 32, 2], 0.0, "xavier").to("cuda")


def test_dropin_nested_compute_gradient_cat_input():
    from pinn_depthestimation_amd.physics import compute_gradient as d
    model = _model()
    N = 500
    g = torch.Generator().manual_seed(2)
    Xh = torch.rand(N, 3, generator=g) * 2 - 1
    t, x, y = [Xh[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(3)]
    u = model(torch.cat([t, x, y], -1))[:, 0:1]
    u_x, u_y = d(u, x), d(u, y)
    u_xx, u_yy = d(u_x, x), d(u_y, y)
    u_xy, u_yx = d(u_x, y), d(u_y, x)
    assert torch.equal(u_xy, u_yx)
    with pytest.raises(PinnError, match="third-order"):
        d(u_xx, x)
    loss = ((d(u, t) - NU * (u_xx + u_yy)) ** 2).mean()
    model.zero_grad()
    loss.backward()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu()
    p64 = [q.detach().double().cpu().requires_grad_(True) for q in model.parameters()]
    cols = [Xh[:, i:i + 1].double().requires_grad_(True) for i in range(3)]
    ref = _heat_residual_ref(p64, cols)
    assert abs(loss.item() - float(ref)) / float(ref) < TOL2
    assert rel_l2(got, O.flat_grad(ref, p64)) < TOL2
    # the second derivatives themselves
    uref = O.mlp_forward(p64, torch.cat(cols, -1))[:, 0:1]
    ux_ref = O.compute_gradient(uref, cols[1])
    assert rel_l2(u_xx, O.compute_gradient(ux_ref, cols[1])) < TOL2
    assert rel_l2(u_xy, O.compute_gradient(ux_ref, cols[2])) < TOL2


def test_dropin_nested_compute_gradient_leaf_matrix():
    from pinn_depthestimation_amd.physics import compute_gradient as d
    model = _model(seed=4)
    model.set_grad_columns([0, 1, 2])
    N = 300
    g = torch.Generator().manual_seed(9)
    Xh = torch.rand(N, 3, generator=g) * 2 - 1
    X = Xh.clone().cuda().requires_grad_(True)
    u = model(X)[:, 0:1]
    gu = d(u, X)                                 # (N, 3): u_t, u_x, u_y
    H_x, H_y = d(gu[:, 1:2], X), d(gu[:, 2:3], X)
    assert torch.equal(H_x[:, 2:3], H_y[:, 1:2])   # u_xy == u_yx
    with pytest.raises(PinnError, match="third-order"):
        d(H_x[:, 1:2], X)
    loss = ((gu[:, 0:1] - NU * (H_x[:, 1:2] + H_y[:, 2:3])) ** 2).mean()
    model.zero_grad()
    loss.backward()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu()
    p64 = [q.detach().double().cpu().requires_grad_(True) for q in model.parameters()]
    ref = _heat_residual_ref(p64, [Xh[:, i:i + 1].double().requires_grad_(True) for i in range(3)])
    assert abs(loss.item() - float(ref)) / float(ref) < TOL2
    assert rel_l2(got, O.flat_grad(ref, p64)) < TOL2


def test_first_order_step_makes_no_jet2_call_and_matches_jet_backward(monkeypatch):
    """physics_equation(corrected=True) runs through compute_gradient under create_graph: its training step must
    not touch the second-order entries, and its parameter gradient is exactly what the first-order reverse sweeps
    (jet_backward) return for the adjoints autograd hands them."""
    from pinn_depthestimation_amd import physics
    from pinn_depthestimation_amd.dnn import DNN

    def boom(*a, **k):
        raise AssertionError("second-order kernel called on a first-order loss")

    monkeypatch.setattr(Engine, "forward_jet2", boom)
    monkeypatch.setattr(Engine, "jet2_backward", boom)
    seen = []
    orig = Engine.jet_backward

    def spy(self, params, X, gY, gdY, grad):
        seen.append((self, params.clone(), X.clone(), None if gY is None else gY.clone(),
                     None if gdY is None else gdY.clone()))
        return orig(self, params, X, gY, gdY, grad)

    monkeypatch.setattr(Engine, "jet_backward", spy)
    torch.manual_seed(3)
    model = DNN([2, 24, 24, 24, 6], 0.0, "xavier").to("cuda")
    with torch.no_grad():
        model.layers.layer_3.bias[4] = 0.2
        model.layers.layer_3.bias[5] = 1.0
        model.layers.layer_3.bias[0] = 2.0
    g = torch.Generator().manual_seed(5)
    Xh = torch.rand(400, 2, generator=g) * 2 - 1
    x, y = [Xh[:, i:i + 1].clone().cuda().requires_grad_(True) for i in range(2)]
    pred = model(torch.cat([x, y], -1))
    loss = physics.physics_equation(x, y, *[pred[:, i:i + 1] for i in range(6)], corrected=True)
    model.zero_grad()
    loss.backward()
    assert torch.isfinite(loss)
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    assert 1 <= len(seen) <= 2
    acc = None
    for eng, params, X, gY, gdY in seen:
        part = orig(eng, params, X, gY, gdY, torch.zeros_like(params))
        acc = part if acc is None else acc + part
    assert torch.equal(got, acc)

"""Parity of the wide MFMA engine (64 < hidden width <= 256, one launch per layer — the shape
class of BASELINE configs[3], 12 x 256) against the fp64 oracle and the generic engine."""
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import ENGINE_GENERIC, ENGINE_WIDE
from tests.golden_util import oracle_loss_and_grad, rel_l2

pytestmark = pytest.mark.gpu

CASES = {
    "ns_3x128": (3, 4, 3, 128, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),
    "ns_2x256": (3, 4, 2, 256, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),
    "pe_3x100": (2, 6, 3, 100, (0, 1), "physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")),
    "co_2x200": (2, 3, 2, 200, (0, 1), "continuity_only", ("x", "y"), ("U", "V", "h")),
    # output column 0 is not a role of the residual (round-3 regression, see test_engine_gpu.py)
    "ns_out_first_2x128": (3, 6, 2, 128, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("aux0", "h", "z", "u", "aux1", "v")),
}


def make(name, N, seed=4321):
    return make_case(CASES[name], N, seed)


def make_case(case, N, seed=4321):
    d_in, d_out, L, W, gc, res, inn, outn = case
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(O.layer_sizes(d_in, L, W, d_out), "xavier", g)
    if res == "physics_equation":
        params[-1][outn.index("h")] = 0.75
        params[-1][outn.index("eta_mean")] = 0.0
    X = torch.rand(N, d_in, generator=g) * 2 - 1
    return params, X, NetDesc(d_in, d_out, L, W, gc), res, inn, outn


@pytest.mark.parametrize("name", list(CASES))
def test_wide_loss_grad_and_jet(name):
    N = 1237
    params, X, desc, res, inn, outn = make(name, N)
    if res == "continuity_only":
        X[:, 0] = X[:, 0] * 40
    eng = Engine(desc.with_(engine=ENGINE_WIDE))
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    l64, g64 = oracle_loss_and_grad(params, X, res, inn, outn, desc.grad_cols, torch.float64)
    l32, g32 = oracle_loss_and_grad(params, X, res, inn, outn, desc.grad_cols, torch.float32)
    if res == "continuity_only":
        cnt = float((X[:, 0] < 25.5).sum())
        scale = torch.tensor([1.0 / N, 1.0 / cnt, 0.0])
    else:
        scale = torch.full((spec.n_terms,), 1.0 / N)
    grad = torch.zeros(desc.n_params, device="cuda")
    sums = eng.residual_loss_grad(spec, scale.cuda(), flat, Xd, grad)
    loss = float((sums.cpu().double() * scale.double()).sum())
    assert abs(loss - float(l64)) / abs(float(l64)) < max(3e-6, 4 * abs(float(l32) - float(l64)) / abs(float(l64)))
    assert rel_l2(grad.cpu(), g64) < max(3e-5, 4 * rel_l2(g32, g64))
    assert torch.allclose(eng.residual_loss(spec, flat, Xd), sums, rtol=1e-6)
    Y, dY = eng.forward_jet(flat, Xd)
    Yo, dYo = O.jet([p.double() for p in params], X.double(), desc.grad_cols)
    assert (Y.cpu().double() - Yo).abs().max() < 3e-6
    assert (dY.cpu().double() - dYo).abs().max() < 3e-6 * max(1.0, float(dYo.abs().max()))
    assert (eng.forward(flat, Xd).cpu().double() - Yo).abs().max() < 3e-6


def test_wide_mse_and_auto_dispatch():
    params, X, desc, *_ = make("ns_3x128", 50)
    g = torch.Generator().manual_seed(2)
    T = torch.rand(50, 2, generator=g)
    p = [q.double().requires_grad_(True) for q in params]
    lo = O.fidelity_loss(p, X.double(), T.double(), [2, 0], [1.0, 3.0])
    go = O.flat_grad(lo, p)
    eng = Engine(desc)                                     # AUTO must pick the wide engine for width 128
    scale = torch.tensor([1.0, 3.0]) / 50
    grad = torch.zeros(desc.n_params, device="cuda")
    sums = eng.mse_loss_grad(O.flatten(params).cuda(), X.cuda(), T.cuda(), [2, 0], scale.cuda(), grad)
    assert abs(float((sums.cpu().double() * scale.double()).sum()) - float(lo)) / float(lo) < 3e-6
    assert rel_l2(grad.cpu(), go) < 3e-5
    gen = Engine(desc.with_(engine=ENGINE_GENERIC))
    grad2 = torch.zeros(desc.n_params, device="cuda")
    gen.mse_loss_grad(O.flatten(params).cuda(), X.cuda(), T.cuda(), [2, 0], scale.cuda(), grad2)
    assert rel_l2(grad.cpu(), grad2.cpu()) < 3e-5


def test_wide_chunked_12x256_matches_generic():
    """BASELINE configs[3] shape; enough points that the host loop runs several chunks."""
    desc = NetDesc(3, 4, 12, 256, (0, 1, 2))
    g = torch.Generator().manual_seed(11)
    params = O.flatten(O.init_params(desc.layers, "xavier", g)).cuda()
    N = 120_011
    X = (torch.rand(N, 3, generator=g) * 2 - 1).cuda()
    spec = ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), desc.grad_cols, ("h", "z", "u", "v"))
    scale = torch.full((3,), 1.0 / N, device="cuda")
    gw, gg = torch.zeros(desc.n_params, device="cuda"), torch.zeros(desc.n_params, device="cuda")
    sw = Engine(desc.with_(engine=ENGINE_WIDE)).residual_loss_grad(spec, scale, params, X, gw)
    sg = Engine(desc.with_(engine=ENGINE_GENERIC)).residual_loss_grad(spec, scale, params, X, gg)
    assert torch.allclose(sw, sg, rtol=3e-5)
    assert rel_l2(gw.cpu(), gg.cpu()) < 3e-5


def test_wide_bf16_mfma_mode():
    """PINN_PREC_BF16 (BASELINE configs[3]: bf16 MFMA, fp32 accumulate / residual): hidden-layer
    GEMM operands are rounded to bf16 (8-bit mantissa), so the tolerance is 2e-2 on the loss and
    5e-2 (relative L2) on the gradient against the fp64 oracle; the fp32 mode of the same engine
    is the bit-for-bit-class reference (3e-6 / 3e-5 above)."""
    from pinn_depthestimation_amd._lib import PREC_BF16
    N = 2000
    params, X, desc, res, inn, outn = make("ns_2x256", N)
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    l64, g64 = oracle_loss_and_grad(params, X, res, inn, outn, desc.grad_cols, torch.float64)
    eng = Engine(desc.with_(precision=PREC_BF16))
    scale = torch.full((3,), 1.0 / N, device="cuda")
    grad = torch.zeros(desc.n_params, device="cuda")
    sums = eng.residual_loss_grad(spec, scale, flat, Xd, grad)
    loss = float((sums * scale).sum())
    el, eg = abs(loss - float(l64)) / float(l64), rel_l2(grad.cpu(), g64)
    print(f"bf16 mode: loss rel err {el:.2e}, grad rel-L2 err {eg:.2e}")
    assert el < 2e-2 and eg < 5e-2
    assert el > 1e-6            # it really is the reduced-precision path
    # narrow networks have no bf16 path: loud refusal, no silent fp32
    from pinn_depthestimation_amd import PinnError
    with pytest.raises(PinnError, match="bf16"):
        Engine(NetDesc(3, 4, 8, 64, (0, 1, 2), precision=PREC_BF16)).forward(torch.zeros(29636, device="cuda"), Xd)


def test_wide_bf16_unfolded_first_layer_width_129():
    """bf16 mode at padded width 256 with more than three inputs: the first layer is NOT folded into the forward chain kernel
    (k_chain_fwd8<16, K1, false>), at K1 = 3 through a residual request and at K1 = 1 through the fidelity term (which takes no
    input derivatives) — the two launcher arms no other test of the wide and chain engines reaches.  The smallest shape that
    takes them: two hidden layers (one W x W matrix), width 129, N = 17 (a full tile and a partial one), d_in = 4; d_out = 6
    puts the output layer's reverse pass on the per-layer kernels as well.  Tolerances: test_wide_bf16_mfma_mode's."""
    from pinn_depthestimation_amd._lib import PREC_BF16
    N = 17
    case = (4, 6, 2, 129, (0, 1), "physics_equation", ("x", "y", "a", "b"), ("h", "U", "V", "eta_mean", "Hrms", "k"))
    params, X, desc, res, inn, outn = make_case(case, N)
    # the wide engine by name, so that no later dispatch rule can route this shape elsewhere and leave the test passing
    eng = Engine(desc.with_(engine=ENGINE_WIDE, precision=PREC_BF16))
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    # K1 = 3: the residual and its gradient
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    l64, g64 = oracle_loss_and_grad(params, X, res, inn, outn, desc.grad_cols, torch.float64)
    scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
    grad = torch.zeros(desc.n_params, device="cuda")
    sums = eng.residual_loss_grad(spec, scale, flat, Xd, grad)
    el, eg = abs(float((sums * scale).sum()) - float(l64)) / float(l64), rel_l2(grad.cpu(), g64)
    print(f"bf16 mode, unfolded first layer, K1 = 3: loss rel err {el:.2e}, grad rel-L2 err {eg:.2e}")
    assert el < 2e-2 and eg < 5e-2
    assert el > 1e-6            # it really is the reduced-precision path (as in test_wide_bf16_mfma_mode)
    # K1 = 1: the fidelity term and its gradient
    T = torch.rand(N, 2, generator=torch.Generator().manual_seed(2))
    p = [q.double().requires_grad_(True) for q in params]
    lo = O.fidelity_loss(p, X.double(), T.double(), [2, 0], [1.0, 3.0])
    go = O.flat_grad(lo, p)
    wts = torch.tensor([1.0, 3.0]) / N
    grad.zero_()
    sums = eng.mse_loss_grad(flat, Xd, T.cuda(), [2, 0], wts.cuda(), grad)
    el, eg = abs(float((sums.cpu().double() * wts.double()).sum()) - float(lo)) / float(lo), rel_l2(grad.cpu(), go)
    print(f"bf16 mode, unfolded first layer, K1 = 1: loss rel err {el:.2e}, grad rel-L2 err {eg:.2e}")
    assert el < 2e-2 and eg < 5e-2
    assert el > 1e-6

"""The tile kernel (k_fused, PINN_ENGINE_FUSED_TILE) with its memory and LDS instructions issued from slots between the MFMAs
(fused_kernel.h: gemm_stream's weight, bias and spill operations; weight_grad's transposes dealt over the preceding quantity's
MFMAs).  The arithmetic is untouched, so the bars are the ones of tests/test_fused_diet_gpu.py, built the same way; what
these cases add is the shapes at which the SLOT arithmetic can go wrong:

  ns_1x64   3 -> 1x64 -> 4    no hidden loop: only the output GEMM's gemm_stream<NTH, 1>, MID_BLOCK = 0
  ns_2x64   3 -> 2x64 -> 4    each layer loop runs once
  ns_8x64   3 -> 8x64 -> 4    the headline instance
  ns_12x64  3 -> 12x64 -> 4   gradient copy in global memory
  cf_2x20   2 -> 2x20 -> 3    NT = 2: 24 MFMAs per block for 6 + 2 operations (+ 2 bias loads in block 0)
  ns_3x12   3 -> 3x12 -> 4    NT = 1: 16 MFMAs per block (8 slots for 1 + 1 + 4 operations), 4 MFMAs per weight-gradient quantity
                              for 6 LDS operations: more operations than MFMAs to put them in front of
  pe_3x10   2 -> 3x10 -> 6    NT = 1, K1 = 3: 12 MFMAs per block
  one jet_backward request at width 64 (EPI_ADJ); a loss-only request on every width-64 net (GRAD = false: no spill operations).

Point counts (C = number of CUs; one workgroup of four waves per CU, one 16-point tile per wave and pass): N = 5 (one ragged
tile), 16 * 4 * C + 5 (every wave one tile, one wave a ragged second one), 2 * 16 * 4 * C + 5 (every wave loops; the four waves
of a workgroup contend for the layer locks).  ns_12x64 leaves out the last.

Bars: loss 2e-6 relative against the fp64 oracle, gradient 2e-5 relative L2, each widened only to 4x the oracle's own
fp32-vs-fp64 distance where that is larger; twice that against the generic engine (another fp32 evaluation with another
summation order: both sit within their bar of the oracle).  The oracle runs on the GPU in fp64 and fp32, once per (net, N).
"""
import functools

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import ENGINE_FUSED_TILE, ENGINE_GENERIC

from tests.golden_util import oracle_loss_and_grad, rel_l2

pytestmark = pytest.mark.gpu

NS = ((0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"))
NETS = {
    # name: (d_in, d_out, hidden, width, grad_cols, residual, in names, out names)
    "ns_1x64": (3, 4, 1, 64) + NS,
    "ns_2x64": (3, 4, 2, 64) + NS,
    "ns_8x64": (3, 4, 8, 64) + NS,
    "ns_12x64": (3, 4, 12, 64) + NS,
    "cf_2x20": (2, 3, 2, 20, (0, 1), "continuity_ftemp", ("x", "y"), ("U", "V", "h")),
    "ns_3x12": (3, 4, 3, 12) + NS,
    "pe_3x10": (2, 6, 3, 10, (0, 1), "physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")),
}
POINTS = {
    "one_partial_tile": lambda cus: 5,
    "one_tile_per_wave": lambda cus: 16 * 4 * cus + 5,
    "two_tiles_per_wave": lambda cus: 2 * 16 * 4 * cus + 5,
}
CASES = [(net, pts) for net in NETS for pts in POINTS if not (net == "ns_12x64" and pts == "two_tiles_per_wave")]


def n_points(pts):
    return POINTS[pts](torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def evaluate(net, pts):
    """Everything the loss-and-gradient tests compare, computed once: two calls of the tile kernel, one loss-only call, one of
    the generic engine, the oracle in fp64 and fp32."""
    d_in, d_out, L, W, gc, res, inn, outn = NETS[net]
    N = n_points(pts)
    g = torch.Generator().manual_seed(50210 + N % 997)
    params = O.init_params(O.layer_sizes(d_in, L, W, d_out), "xavier", g)
    X = (torch.rand(N, d_in, generator=g) * 2 - 1).cuda().contiguous()
    flat = O.flatten(params).cuda()
    desc = NetDesc(d_in, d_out, L, W, gc)
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
    out = {"N": N, "scale": scale.cpu().double()}
    for key, engine in (("tile", ENGINE_FUSED_TILE), ("tile_again", ENGINE_FUSED_TILE), ("generic", ENGINE_GENERIC)):
        eng = Engine(desc.with_(engine=engine))
        grad = torch.zeros(desc.n_params, device="cuda")
        sums = eng.residual_loss_grad(spec, scale, flat, X, grad)
        out[key] = (sums.cpu().clone(), grad.cpu().clone())
    if W == 64:   # GRAD = false: the same streams without the spill operations
        sums = Engine(desc.with_(engine=ENGINE_FUSED_TILE)).residual_loss(spec, flat, X)
        out["tile_loss_only"] = (sums.cpu().clone(), None)
    dev_params = [p.cuda() for p in params]
    for key, dtype in (("o64", torch.float64), ("o32", torch.float32)):
        loss, grad = oracle_loss_and_grad(dev_params, X, res, inn, outn, desc.grad_cols, dtype)
        out[key] = (float(loss), grad.cpu().double())
    return out


def bars(r):
    l64, g64 = r["o64"]
    l32, g32 = r["o32"]
    return max(2e-6, 4 * abs(l32 - l64) / abs(l64)), max(2e-5, 4 * rel_l2(g32, g64))


def loss_of(r, key):
    return float((r[key][0].double() * r["scale"]).sum())


@pytest.mark.parametrize("net,pts", CASES)
def test_paced_tile_kernel_matches_fp64_oracle(net, pts):
    r = evaluate(net, pts)
    loss_bar, grad_bar = bars(r)
    l64, g64 = r["o64"]
    loss_err, grad_err = abs(loss_of(r, "tile") - l64) / abs(l64), rel_l2(r["tile"][1], g64)
    print(f"{net} N={r['N']}: loss err {loss_err:.2e} (bar {loss_bar:.1e}), gradient err {grad_err:.2e} (bar {grad_bar:.1e})")
    assert loss_err < loss_bar
    assert grad_err < grad_bar


@pytest.mark.parametrize("net,pts", CASES)
def test_paced_tile_kernel_matches_generic_engine(net, pts):
    r = evaluate(net, pts)
    loss_bar, grad_bar = bars(r)
    lt, lg = loss_of(r, "tile"), loss_of(r, "generic")
    loss_d, grad_d = abs(lt - lg) / abs(lg), rel_l2(r["tile"][1], r["generic"][1])
    print(f"{net} N={r['N']}: loss tile vs generic {loss_d:.2e}, gradient {grad_d:.2e}")
    assert loss_d < 2 * loss_bar
    assert grad_d < 2 * grad_bar


@pytest.mark.parametrize("net,pts", [(net, pts) for net, pts in CASES if NETS[net][3] == 64])
def test_loss_only_request_at_width_64(net, pts):
    """GRAD = false: forward streams with weight and bias operations only."""
    r = evaluate(net, pts)
    loss_bar, _ = bars(r)
    l64 = r["o64"][0]
    loss_err = abs(loss_of(r, "tile_loss_only") - l64) / abs(l64)
    loss_d = abs(loss_of(r, "tile_loss_only") - loss_of(r, "generic")) / abs(loss_of(r, "generic"))
    print(f"{net} N={r['N']} loss only: err {loss_err:.2e} (bar {loss_bar:.1e}), vs generic {loss_d:.2e}")
    assert loss_err < loss_bar
    assert loss_d < 2 * loss_bar


@functools.lru_cache(maxsize=None)
def evaluate_jet_backward(pts):
    """grad of sum(gY * Y) + sum(gdY * dY) on the headline net: tile kernel twice, generic engine, autograd in fp64 and fp32."""
    d_in, d_out, L, W, gc = 3, 4, 8, 64, (0, 1, 2)
    N = n_points(pts)
    g = torch.Generator().manual_seed(60310 + N % 997)
    desc = NetDesc(d_in, d_out, L, W, gc)
    params = O.init_params(desc.layers, "xavier", g)
    X = (torch.rand(N, d_in, generator=g) * 2 - 1).cuda().contiguous()
    gY = torch.randn(N, d_out, generator=g).cuda()
    gdY = torch.randn(desc.k, N, d_out, generator=g).cuda()
    flat = O.flatten(params).cuda()
    out = {"N": N}
    for key, engine in (("tile", ENGINE_FUSED_TILE), ("tile_again", ENGINE_FUSED_TILE), ("generic", ENGINE_GENERIC)):
        eng = Engine(desc.with_(engine=engine))
        if engine == ENGINE_FUSED_TILE:
            assert eng.jet_backward_kernel(N) == ENGINE_FUSED_TILE
        grad = torch.zeros(desc.n_params, device="cuda")
        eng.jet_backward(flat, X, gY, gdY, grad)
        out[key] = grad.cpu().clone()
    for key, dtype in (("o64", torch.float64), ("o32", torch.float32)):
        p = [q.cuda().to(dtype).clone().requires_grad_(True) for q in params]
        cols = O.split_columns(X.to(dtype), desc.grad_cols)
        Y = O.mlp_forward(p, torch.cat(cols, -1), "xavier")
        dY = torch.stack([torch.cat([O.compute_gradient(Y[:, c:c + 1], cols[j]) for c in range(d_out)], 1) for j in gc])
        out[key] = O.flat_grad((gY.to(dtype) * Y).sum() + (gdY.to(dtype) * dY).sum(), p).cpu().double()
    return out


@pytest.mark.parametrize("pts", sorted(POINTS))
def test_jet_backward_request_at_width_64(pts):
    """EPI_ADJ: the caller's adjoints instead of a residual epilogue, the same streams and weight gradient."""
    r = evaluate_jet_backward(pts)
    grad_bar = max(2e-5, 4 * rel_l2(r["o32"], r["o64"]))
    grad_err, grad_d = rel_l2(r["tile"], r["o64"]), rel_l2(r["tile"], r["generic"])
    print(f"jet_backward 8x64 N={r['N']}: gradient err {grad_err:.2e} (bar {grad_bar:.1e}), vs generic {grad_d:.2e}")
    assert grad_err < grad_bar
    assert grad_d < 2 * grad_bar


@pytest.mark.parametrize("net", sorted(NETS))
def test_one_tile_pass_is_bitwise_reproducible(net):
    """One tile = one wave of one workgroup: nothing races for the gradient copy, so two calls agree in every bit."""
    r = evaluate(net, "one_partial_tile")
    assert torch.equal(r["tile"][0], r["tile_again"][0])
    assert torch.equal(r["tile"][1], r["tile_again"][1])


def test_one_tile_jet_backward_is_bitwise_reproducible():
    r = evaluate_jet_backward("one_partial_tile")
    assert torch.equal(r["tile"], r["tile_again"])

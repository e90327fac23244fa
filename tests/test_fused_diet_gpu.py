"""The tile kernel (k_fused, PINN_ENGINE_FUSED_TILE) at the point counts where its wave loop and its gradient lock change
behaviour, after the instruction diet of fused_kernel.h (packed activation, unit tangents of layer 0 built in operand layout,
bias row sums by row swaps, the bias values read with the flush, output tiles kept out of scratch memory).

Point counts (C = number of CUs; the width-64 gradient kernel runs one workgroup of four waves per CU, one 16-point tile per
wave and pass):
  one_partial_tile   N = 5                 one ragged tile, one wave of one workgroup: no lock contention, reproducible
  one_tile_per_wave  N = 16 * 4 * C + 5    every wave gets one tile and one wave a ragged second one
  two_tiles_per_wave N = 2 * 16 * 4 * C + 5  every wave loops, the four waves of a workgroup contend for the layer locks

Bars: those of tests/test_engine_gpu.py for this kernel — loss 2e-6 relative against the fp64 oracle, gradient 2e-5 relative
L2, each widened only to 4x the oracle's own fp32-vs-fp64 distance where that is larger.  Against the generic engine (another
fp32 evaluation of the same quantities with another summation order) the bar is the sum of the two engines' bars: both sit
within their bar of the fp64 oracle.  The oracle (oracle/pinn_oracle.py, plain torch) is evaluated on the GPU in fp64 and
fp32: on the CPU its double-backward takes tens of seconds at these N.  One evaluation per (net, N) is shared by all tests.
"""
import functools

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import ENGINE_FUSED_TILE, ENGINE_GENERIC

from tests.golden_util import oracle_loss_and_grad, rel_l2

pytestmark = pytest.mark.gpu

NETS = {
    # name: (d_in, d_out, hidden, width, grad_cols, residual, in names, out names)
    "ns_8x64": (3, 4, 8, 64, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),   # the headline instance
    "cf_2x20": (2, 3, 2, 20, (0, 1), "continuity_ftemp", ("x", "y"), ("U", "V", "h")),             # padded width 32
    "cf_40x20": (2, 3, 40, 20, (0, 1), "continuity_ftemp", ("x", "y"), ("U", "V", "h")),           # width 32, gradient copy in global memory
    "ns_3x12": (3, 4, 3, 12, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),   # padded width 16
}
POINTS = {
    "one_partial_tile": lambda cus: 5,
    "one_tile_per_wave": lambda cus: 16 * 4 * cus + 5,
    "two_tiles_per_wave": lambda cus: 2 * 16 * 4 * cus + 5,
}
CASES = [(net, pts) for net in ("ns_8x64", "cf_2x20", "ns_3x12") for pts in POINTS] + [("cf_40x20", "one_partial_tile"),
                                                                                      ("cf_40x20", "one_tile_per_wave")]


@functools.lru_cache(maxsize=None)
def evaluate(net, pts):
    """Everything the tests compare, computed once: two calls of the tile kernel, one of the generic engine, the oracle."""
    d_in, d_out, L, W, gc, res, inn, outn = NETS[net]
    N = POINTS[pts](torch.cuda.get_device_properties(0).multi_processor_count)
    g = torch.Generator().manual_seed(20240 + N % 997)
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
def test_tile_kernel_matches_fp64_oracle(net, pts):
    r = evaluate(net, pts)
    loss_bar, grad_bar = bars(r)
    l64, g64 = r["o64"]
    loss_err, grad_err = abs(loss_of(r, "tile") - l64) / abs(l64), rel_l2(r["tile"][1], g64)
    print(f"{net} N={r['N']}: loss err {loss_err:.2e} (bar {loss_bar:.1e}), gradient err {grad_err:.2e} (bar {grad_bar:.1e})")
    assert loss_err < loss_bar
    assert grad_err < grad_bar


@pytest.mark.parametrize("net,pts", CASES)
def test_tile_kernel_matches_generic_engine(net, pts):
    r = evaluate(net, pts)
    loss_bar, grad_bar = bars(r)
    lt, lg = loss_of(r, "tile"), loss_of(r, "generic")
    loss_d, grad_d = abs(lt - lg) / abs(lg), rel_l2(r["tile"][1], r["generic"][1])
    print(f"{net} N={r['N']}: loss tile vs generic {loss_d:.2e}, gradient {grad_d:.2e}")
    assert loss_d < 2 * loss_bar
    assert grad_d < 2 * grad_bar


@pytest.mark.parametrize("net", sorted(NETS))
def test_one_tile_pass_is_bitwise_reproducible(net):
    """One tile = one wave of one workgroup: nothing races for the gradient copy, so two calls agree in every bit."""
    r = evaluate(net, "one_partial_tile")
    assert torch.equal(r["tile"][0], r["tile_again"][0])
    assert torch.equal(r["tile"][1], r["tile_again"][1])

"""Seeded random sweep of the second-order jet entries over width, depth, k, direction columns, d_out, N and activation:
the MFMA kernels (FUSED, every case with all layers at most 64 wide) against the generic kernels, and one case in five
against fp64 torch double-backward."""
import random

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc
from pinn_depthestimation_amd._lib import ACT_LEAKY_RELU, ACT_TANH, ENGINE_FUSED, ENGINE_GENERIC
from tests.test_jet2_gpu import TOL1, TOL2, ref_grad, ref_jets, rel_l2

pytestmark = pytest.mark.gpu


def _cases(n=20, seed=2024):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        d_in = rng.randint(1, 4)
        k = rng.randint(1, min(3, d_in))
        cols = tuple(rng.sample(range(d_in), k))
        act = rng.choice([ACT_TANH, ACT_TANH, ACT_LEAKY_RELU])
        desc = NetDesc(d_in, rng.randint(1, 7), rng.randint(1, 6), rng.choice([5, 8, 16, 20, 33, 64, 100]), cols,
                       activation=act)
        out.append((i, desc, rng.choice([1, 16, 31, 200, 257, 640])))
    return out


@pytest.mark.parametrize("i,desc,N", _cases(), ids=lambda v: str(v) if isinstance(v, int) else None)
def test_jet2_sweep(i, desc, N):
    init = "kaiming" if desc.activation == ACT_LEAKY_RELU else "xavier"
    g = torch.Generator().manual_seed(100 + i)
    params = O.init_params(desc.layers, init, g)
    X = torch.rand(N, desc.d_in, generator=g) * 2 - 1
    flat, Xc = O.flatten(params).cuda(), X.cuda()
    P = desc.k * (desc.k + 1) // 2
    adj = (torch.randn(N, desc.d_out, generator=g), torch.randn(desc.k, N, desc.d_out, generator=g),
           torch.randn(P, N, desc.d_out, generator=g))
    mfma = desc.width <= 64
    res = {}
    for e in (ENGINE_GENERIC, ENGINE_FUSED) if mfma else (ENGINE_GENERIC,):
        eng = Engine(desc.with_(engine=e), "cuda")
        Y, dY, d2Y = eng.forward_jet2(flat, Xc)
        grad = torch.zeros_like(flat)
        eng.jet2_backward(flat, Xc, *[a.cuda() for a in adj], grad)
        res[e] = (Y, dY, d2Y, grad)
    if mfma:                                         # fp32 rounding apart (MFMA sums in another order)
        for a, b in zip(res[ENGINE_FUSED], res[ENGINE_GENERIC]):
            assert rel_l2(a, b) < 5e-6, (i, rel_l2(a, b))
    if i % 5:
        return
    p64, Yr, dYr, d2Yr = ref_jets(params, X, desc.grad_cols, init)
    for e, (Y, dY, d2Y, grad) in res.items():
        assert rel_l2(Y, Yr) < TOL1 and rel_l2(dY, dYr) < TOL1
        if desc.activation == ACT_TANH:
            assert rel_l2(d2Y, d2Yr) < TOL2
        else:                                        # LeakyReLU: every second derivative is exactly zero
            assert float(d2Y.abs().max()) == 0.0 and float(d2Yr.abs().max()) == 0.0
        assert rel_l2(grad, ref_grad(p64, Yr, dYr, d2Yr, *adj)) < TOL2

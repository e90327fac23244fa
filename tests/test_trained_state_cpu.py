"""The reference side of tests/test_trained_state_gpu.py, without a GPU: that the recipe of tests/trained_state_util.py
gives what it says, that the oracle's own fp32-vs-fp64 gap stays under the cap in every block of every case the GPU module
uses, and that the per-block comparison REJECTS what a kernel that mis-reads hidden biases would compute — so the GPU
tests can fail.

Measured on the oracle at N = 777, seed 1234 (every (case, state) of trained_state_util.LOSS_GRAD):
  the oracle's fp32-vs-fp64 gap per block      at most 2.4e-7 (biased), 4.9e-7 (saturating)
  hidden biases dropped                        every block off by >= 1.1e-1, loss by >= 1.7e-2
  hidden biases rolled by one unit             every block off by >= 1.4e-1, loss by >= 3.1e-2
  the last hidden layer's bias dropped         every block off by >= 6.5e-2, loss by >= 5.7e-3
  one unit's bias dropped (last unit of the
  middle layer)                                every block off by >= 2.0e-3 (pe_8x64), loss by >= 2.1e-4 (ns_5in)
against a per-block bound of 2e-5 and a loss bound of 2e-6: no mutant's loss is insensitive, so every one is asserted on
the gradient AND on the loss."""
import pytest
import torch

from oracle import pinn_oracle as O
from tests import trained_state_util as U
from tests.golden_util import rel_l2

MUTANT_CASES = ["ns_8x64", "ns_3x12", "pe_10x10", "pe_8x64", "cf_3x32", "cf_40x20", "co_3x64", "ns_3x128"]


def _last_hidden(c):
    a = c.X.double()
    for i in range(c.L):
        a = torch.tanh(a @ c.params[2 * i].double().t() + c.params[2 * i + 1].double())
    return a


# ---- the recipe -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pe_10x10", "ns_3x12", "co_3x64"])
def test_recipe(name):
    d_in, d_out, L, W, gc, res, inn, outn = U.CASES[name]
    layers = O.layer_sizes(d_in, L, W, d_out)
    a = U.trained_like(layers, torch.Generator().manual_seed(5), residual=res, outn=outn)
    b = U.trained_like(layers, torch.Generator().manual_seed(5), residual=res, outn=outn)
    plain = O.init_params(layers, "xavier", torch.Generator().manual_seed(5))
    assert len(a) == 2 * (L + 1) and all(torch.equal(p, q) for p, q in zip(a, b))          # the same seed, the same parameters
    for i in range(L):
        bias = a[2 * i + 1]
        assert bias.shape == (W,) and bool((bias != 0).all()) and float(bias.abs().max()) <= 0.5 and float(bias.abs().max()) > 0.25
        assert torch.equal(a[2 * i], plain[2 * i])                                           # gain 1: the Xavier weights
        assert len(set(bias.tolist())) == W                                                  # no two units share a bias
    s = U.trained_like(layers, torch.Generator().manual_seed(5), residual=res, outn=outn, **U.STATES["saturating"])
    for i in range(L):
        assert torch.equal(s[2 * i], plain[2 * i] * 3.0) and 0.5 < float(s[2 * i + 1].abs().max()) <= 1.0
    if res == "physics_equation":
        assert torch.equal(a[-2], plain[-2] * 0.25)
        assert [float(a[-1][outn.index(r)]) for r in ("h", "eta_mean", "k")] == [0.75, 0.0, 0.5]
    else:
        assert torch.equal(a[-2], plain[-2]) and torch.equal(a[-1], plain[-1]) and torch.equal(s[-2], plain[-2])


def test_param_blocks_cover_the_flat_vector_in_order():
    layers = [3, 12, 12, 4]
    blocks = U.param_blocks(layers)
    assert [b[0] for b in blocks] == ["W0", "b0", "W1", "b1", "W2", "b2"]
    assert blocks[0][1] == 0 and all(blocks[i][2] == blocks[i + 1][1] for i in range(5))
    params = [torch.full((layers[i // 2 + 1], layers[i // 2]) if i % 2 == 0 else (layers[i // 2 + 1],), float(i)) for i in range(6)]
    flat = O.flatten(params)
    assert blocks[-1][2] == flat.numel()
    for i, (_, a, b) in enumerate(blocks):
        assert bool((flat[a:b] == i).all()) and b - a == params[i].numel()


@pytest.mark.parametrize("name", [n for n, s in U.LOSS_GRAD if s == "saturating"])
def test_the_saturating_state_saturates(name):
    c = U.Case(name, "saturating")
    sat = float((_last_hidden(c).abs() > 0.99).double().mean())
    print(f"{name}: {100 * sat:.0f} % of the last hidden layer's activations exceed 0.99")
    assert sat > 0.10
    assert float((_last_hidden(U.Case(name, "biased")).abs() > 0.99).double().mean()) < 0.01


def test_the_saturating_state_is_refused_for_deep_networks():
    with pytest.raises(AssertionError, match="saturating"):
        U.Case("ns_8x64", "saturating")


# ---- the cap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,state", U.LOSS_GRAD + [("pe_4x48", "biased"), ("ns_5x256", "biased")])
def test_the_references_own_gap_is_under_the_cap_in_every_block(name, state):
    c, l64, g64, l32, g32 = U.reference(name, state)
    gaps = U.block_errors(g32, g64, c.layers)
    print(f"{name} {state}: largest fp32-fp64 gap {U.worst(gaps)[1]:.1e} in {U.worst(gaps)[0]}, loss {abs(l32 - l64) / abs(l64):.1e}")
    assert all(float(g64[a:b].norm()) > 0 for _, a, b in U.param_blocks(c.layers))          # every block carries gradient
    assert max(gaps.values()) <= U.GAP_CAP
    assert abs(l32 - l64) / abs(l64) < 5e-7                                                  # ... so the loss bound is its 2e-6 floor
    U.assert_blocks_close(g32, g64, g32, c.layers, f"{name} {state}: the reference's own fp32 run")


@pytest.mark.parametrize("name", sorted(U.ENSEMBLE))
def test_the_cap_holds_for_every_ensemble_member(name):
    """The ensemble cases of the GPU module (co_40x20 among them): other seeds, other point counts, one draw per member."""
    c, members, T, refs = U.ensemble_reference(name)
    assert len(members) == U.ENSEMBLE_M and not torch.equal(members[0][1], members[1][1]) and not torch.equal(members[1][1], members[2][1])
    for m, (l64, g64, l32, g32) in enumerate(refs):
        gaps = U.block_errors(g32, g64, c.layers)
        print(f"{name} member {m}: largest fp32-fp64 gap {U.worst(gaps)[1]:.1e} in {U.worst(gaps)[0]}, loss {abs(l32 - l64) / abs(l64):.1e}")
        assert max(gaps.values()) <= U.GAP_CAP and abs(l32 - l64) / abs(l64) < 5e-7
        U.assert_blocks_close(g32, g64, g32, c.layers, f"{name} member {m}: the reference's own fp32 run")


# ---- the mutants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,state", [(n, "biased") for n in MUTANT_CASES] + [("ns_3x12", "saturating"), ("co_3x64", "saturating")])
def test_every_bias_mutant_is_rejected(name, state):
    c, l64, g64, l32, g32 = U.reference(name, state)
    for mname, mparams in U.mutants(c.params).items():
        assert any(not torch.equal(p, q) for p, q in zip(mparams, c.params)), mname
        lm, gm = U.oracle_loss_grad(c, mparams)
        errs = U.block_errors(gm, g64, c.layers)
        print(f"{name} {state}, {mname}: smallest block error {min(errs.values()):.1e}, loss off by {abs(lm - l64) / abs(l64):.1e}")
        with pytest.raises(AssertionError, match="out of bound"):
            U.assert_blocks_close(gm, g64, g32, c.layers, f"{name} {mname}")
        assert min(errs.values()) > 50 * 2e-5, (mname, errs)          # EVERY block rejects it, and not by a hair
        assert not abs(lm - l64) / abs(l64) < U.loss_bound(l64, l32), mname


# ---- the comparator ---------------------------------------------------------------------------------------------------
def test_a_planted_block_error_passes_the_whole_vector_rule_and_fails_the_block_rule():
    c, l64, g64, l32, g32 = U.reference("ns_8x64", "biased")
    share = {k: float(g64[a:b].norm() / g64.norm()) for k, a, b in U.param_blocks(c.layers)}
    k = min(share, key=share.get)
    a, b = next((a, b) for n, a, b in U.param_blocks(c.layers) if n == k)
    assert k.startswith("b") and share[k] < 1e-2, (k, share[k])          # a bias block, under 1 % of the gradient's norm
    planted = g32.clone()
    planted[a:b] *= 1.002
    assert rel_l2(planted, g64) < max(2e-5, 4 * rel_l2(g32, g64))        # the whole-vector rule lets a 0.2 % error through
    with pytest.raises(AssertionError, match=rf"out of bound: {k} "):
        U.assert_blocks_close(planted, g64, g32, c.layers, "planted")
    U.assert_blocks_close(g32, g64, g32, c.layers, "not planted")


def test_the_comparator_names_the_block_lists_all_and_holds_zero_blocks_to_zero():
    layers = [2, 3, 1]
    g64 = torch.tensor([1.0, 2, 3, 4, 5, 6, 0, 0, 0, 1, 1, 1, 2.0], dtype=torch.float64)      # b0 is zero
    U.assert_blocks_close(g64.clone(), g64, g64, layers, "exact")
    off = g64.clone(); off[7] = 1e-9
    with pytest.raises(AssertionError, match="b0 .fp64 block is zero") as e:
        U.assert_blocks_close(off, g64, g64, layers, "zero block")
    assert all(n in str(e.value) for n in ("W0 ", "b0 ", "W1 ", "b1 "))
    noisy = g64.clone(); noisy[0] += 1e-4                                                      # the reference's own gap over the cap
    with pytest.raises(AssertionError, match="badly chosen case"):
        U.assert_blocks_close(g64, g64, noisy, layers, "cap")
    with pytest.raises(AssertionError, match="non-finite"):
        U.assert_blocks_close(torch.full_like(g64, float("nan")), g64, g64, layers, "nan")

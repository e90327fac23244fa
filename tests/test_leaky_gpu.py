"""Seeded sweep of the LeakyReLU (init_type "kaiming") kernels — the tile kernel's loss and loss + gradient instances at
every padded width, K1 = 1 / 3 / 4 and either home of the gradient copy, the cooperative kernel, the plain-forward kernel,
the external-adjoint, field and second-order instances, the generic engine — every result held to the fp64 formula of
tests/leaky_util.py (draws, kink-free points, reference, bounds; tests/test_leaky_cpu.py shows on the CPU that the points
are off the kink, that the draws are well conditioned and that every mis-reading of LeakyReLU fails these bounds).

leaky_util.served restates include/pinn_hip.h: a refusal where it says "served" fails, a success where it says "refused"
fails, and a refusal must leave a pre-filled grad / sums untouched.  The named cases sit ON the kink (exact zeros in z):
torch's convention there is slope 0.01, forward and reverse.  Every test prints one line per case: the shape, the engines
that ran, the worst ratio of an error to its bound (1.0 = at the bound).  DESIGN.md 4.5."""
import ctypes as C

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16, PinnError)
from pinn_depthestimation_amd.engine import _ptr
from tests import leaky_util as K
from tests.trained_state_util import assert_blocks_close, block_errors, param_blocks

pytestmark = pytest.mark.gpu

ENGINE = {"auto": ENGINE_AUTO, "generic": ENGINE_GENERIC, "tile": ENGINE_FUSED_TILE, "coop": ENGINE_FUSED_COOP,
          "batch": ENGINE_FUSED_BATCH, "fused": ENGINE_FUSED, "wide": ENGINE_WIDE}
POISON = 1e30


def desc_of(c, tag, **kw):
    return NetDesc(c.d_in, c.d_out, c.L, c.W, c.gc, activation=ACT_LEAKY_RELU, engine=ENGINE[tag], **kw)


def spec_of(c):
    return ResidualSpec.from_names(c.res, c.inn, c.gc, c.outn, corrected=c.corrected, nu=c.nu) if c.res else None


def attempt(family, c, tag, fn, entry=None, untouched=()):
    """fn()'s result, or None where the header says the request is refused and it was, the `untouched` (tensor, copy) pairs
    still equal."""
    ok = K.served(family, c, tag, entry)
    try:
        out = fn()
    except PinnError as err:
        assert not ok, f"{c.tag()} / {tag} {entry or ''}: refused although include/pinn_hip.h documents it as served: {err}"
        torch.cuda.synchronize()
        for t, copy in untouched:
            assert torch.equal(t, copy), f"{c.tag()} / {tag} {entry or ''}: a refused call wrote to its outputs"
        return None
    assert ok, f"{c.tag()} / {tag} {entry or ''}: served although include/pinn_hip.h documents it as refused"
    torch.cuda.synchronize()
    return out


def gradient_ratio(got, r64, r32, layers, what):
    """assert_blocks_close, and the worst live block's error over its bound max(2e-5, 4 gap)."""
    errs = assert_blocks_close(got, r64.grad, r32.grad, layers, what)
    gaps = block_errors(r32.grad, r64.grad, layers)
    live = [name for name, a, b in param_blocks(layers) if float(r64.grad[a:b].norm()) > 0]
    return max(errs[k] / max(2e-5, 4 * gaps[k]) for k in live)


def check_sums(got, s64, s32, what):
    ratio = K.sum_ratio(got, s64, s32)
    assert ratio <= 1.0, (what, torch.as_tensor(got).tolist(), s64.tolist(), ratio)
    return ratio


def check_fields(got, r64, what):
    ratios = K.field_ratios(got, r64)
    assert max(ratios) <= K.FIELD_BOUND, (what, ratios)
    return max(ratios) / K.FIELD_BOUND


def check_jets(got, ref64, what):
    ratio = K.jet_ratio(got, ref64)
    assert ratio <= 1.0, (what, ratio)
    return ratio


def poisoned(n):
    t = torch.full((max(n, 1),), POISON, device="cuda")[:n]
    return t


# ---- the checks, shared by the seeded and the named cases ------------------------------------------------------------------
def loss_call(eng, c, spec, scale, cs, flat, X, T, grad, ts, csm):
    """The gradient entry of the case's kind: (term sums, column sums)."""
    if c.kind == "residual":
        return eng.residual_loss_grad(spec, scale, flat, X, grad, sums=ts), torch.zeros(0)
    if c.kind == "mse":
        return torch.zeros(0), eng.mse_loss_grad(flat, X, T, c.fid_cols, cs, grad, sums=csm)
    if c.kind == "onepass":
        return eng.residual_mse_loss_grad(spec, scale, T, c.fid_cols, cs, flat, X, grad, term_sums=ts, col_sums=csm)
    return eng.residual_mse_split_loss_grad(spec, scale, T, c.fid_cols, cs, flat, X, c.n_res, grad, term_sums=ts, col_sums=csm)


def check_loss(d, ref, tags):
    c, (r64, r32) = d.case, ref
    spec = spec_of(c)
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    T = None if d.T is None else d.T.cuda()
    scale = torch.tensor(c.term_scale(), device="cuda") if c.res else None
    cs = torch.tensor(c.col_scale(), device="cuda")
    ran, worst = [], 0.0
    for tag in tags:
        eng, what = Engine(desc_of(c, tag)), f"{c.tag()} / {tag}"
        if c.res and c.kind in ("residual", "onepass"):          # the forward-only entry, on all N points
            sums = attempt("loss", c, tag, lambda: eng.residual_loss(spec, flat, X), entry="residual_loss")
            if sums is not None:
                worst = max(worst, check_sums(sums, r64.sums, r32.sums, what + " residual_loss"))
        ok = K.served("loss", c, tag)
        grad = torch.zeros(flat.numel(), device="cuda") if ok else torch.randn(flat.numel(), device="cuda")
        base = grad.clone()
        ts, csm = poisoned(K.N_TERMS[c.res] if c.res else 0), poisoned(len(c.fid_cols))
        out = attempt("loss", c, tag, lambda: loss_call(eng, c, spec, scale, cs, flat, X, T, grad, ts, csm),
                      untouched=[(grad, base), (ts, ts.clone()), (csm, csm.clone())])
        if out is None:
            continue
        if c.res:
            worst = max(worst, check_sums(out[0], r64.sums, r32.sums, what + " term sums"))
        worst = max(worst, check_sums(out[1], r64.cols, r32.cols, what + " column sums"), gradient_ratio(grad, r64, r32, c.layers, what))
        ran.append(tag)
    assert "auto" in ran and "generic" in ran and (("tile" in ran) == (c.W <= 64)), (c.tag(), ran)
    return ran, worst


def check_adj(d, ref, tags):
    c, (r64, r32) = d.case, ref
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    gY = None if c.mode == "gdY" else d.gY.cuda()
    gdY = None if c.mode == "gY" else d.gdY.cuda()
    ran, worst = [], 0.0
    for tag in tags:
        eng, what = Engine(desc_of(c, tag)), f"{c.tag()} / {tag}"
        if K.served("adj", c, tag):
            # the batch kernel has no LeakyReLU instance: the tile kernel at every N (the generic kernels where AUTO falls back)
            want = ENGINE_GENERIC if tag == "generic" or c.W > 64 else ENGINE_FUSED_TILE
            for n in (c.N, 4096, 150001):
                assert eng.jet_backward_kernel(n, with_gdY=gdY is not None) == want, (what, n)
        ok = K.served("adj", c, tag)
        grad = torch.zeros(flat.numel(), device="cuda") if ok else torch.randn(flat.numel(), device="cuda")
        base = grad.clone()
        if attempt("adj", c, tag, lambda: eng.jet_backward(flat, X, gY, gdY, grad), untouched=[(grad, base)]) is None:
            continue
        worst = max(worst, gradient_ratio(grad, r64, r32, c.layers, what))
        ran.append(tag)
    assert "auto" in ran and "generic" in ran and (("tile" in ran) == (c.W <= 64)), (c.tag(), ran)
    return ran, worst


def check_fields_entry(d, ref, tags):
    c, (r64, r32) = d.case, ref
    spec = spec_of(c)
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    nf, N = spec.n_fields, c.N
    ran, worst = [], 0.0
    for tag in tags:
        eng, what = Engine(desc_of(c, tag)), f"{c.tag()} / {tag}"
        buf = torch.full((nf * N + 64,), POISON, device="cuda")          # a guard band behind the output, through the raw entry
        copy = buf.clone()

        def run():
            ws = eng.fields_workspace(spec, N)
            eng._run("pinn_residual_fields", eng.lib.pinn_residual_fields, C.byref(eng._d()), C.byref(spec.c_struct()), _ptr(flat), _ptr(X), N,
                     _ptr(buf), _ptr(ws), ws.numel())
            return buf[:nf * N].view(nf, N)
        F = attempt("fields", c, tag, run, untouched=[(buf, copy)])
        if F is None:
            continue
        assert bool((buf[nf * N:] == POISON).all()), what
        worst = max(worst, check_fields(F, r64, what))
        if c.res == "continuity_only":
            off = d.X[:, c.inn.index("x")] >= K.THRESHOLD
            assert bool((F[1].cpu()[off] == 0).all()), what
        if c.res == "continuity_ftemp":
            assert float(F[1].abs().max()) == 0.0, what
        ran.append(tag)
    assert "auto" in ran and "generic" in ran and (("tile" in ran) == (c.W <= 64)), (c.tag(), ran)
    return ran, worst


def check_fwd(d, ref, tags):
    c, (r64, _) = d.case, ref
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    ran, worst = [], 0.0
    for tag in tags:
        eng, what = Engine(desc_of(c, tag)), f"{c.tag()} / {tag}"
        Y = attempt("fwd", c, tag, lambda: eng.forward(flat, X))
        if Y is None:
            continue
        worst = max(worst, check_jets([Y], r64.jets[:1], what + " forward"))
        if c.k:
            Yj, dY = attempt("fwd", c, tag, lambda: eng.forward_jet(flat, X))
            worst = max(worst, check_jets([Yj, dY], r64.jets, what + " forward_jet"))
        ran.append(tag)
    assert "auto" in ran and "generic" in ran and (("fused" in ran) == (c.W <= 64)), (c.tag(), ran)
    return ran, worst


def check_second(d, ref, tags):
    c, (r64, r32) = d.case, ref
    spec = spec_of(c)
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    scale = torch.tensor(c.term_scale(), device="cuda")
    ran, worst = [], 0.0
    for tag in tags:
        eng, what = Engine(desc_of(c, tag)), f"{c.tag()} / {tag}"
        jets = attempt("second", c, tag, lambda: eng.forward_jet2(flat, X))
        ok = K.served("second", c, tag, "residual2")
        grad = torch.zeros(flat.numel(), device="cuda") if ok else torch.randn(flat.numel(), device="cuda")
        base, ts = grad.clone(), poisoned(3)
        out = attempt("second", c, tag, lambda: eng.residual2_loss_grad(spec, scale, flat, X, grad=grad, fields=True, sums=ts),
                      entry="residual2", untouched=[(grad, base), (ts, ts.clone())])
        assert (jets is None) == (out is None), what
        if out is None:
            continue
        worst = max(worst, check_jets(jets, r64.jets, what + " forward_jet2"), check_sums(out[0], r64.sums, r32.sums, what + " term sums"),
                    check_fields(out[1], r64, what), gradient_ratio(grad, r64, r32, c.layers, what))
        ran.append(tag)
    assert "auto" in ran and "generic" in ran and (("fused" in ran) == (max(c.layers) <= 64)), (c.tag(), ran)
    return ran, worst


def check_adam(d, ref, tags, iterations=2):
    """loss_grad_adam_step: the first gradient against the reference, the second (on the case's second point set) per block
    against the oracle at the parameters the first iteration left on the device, the parameters after all iterations against
    Adam steps of the oracle in float64, in units of the step (tests/test_trained_state_gpu.py's rule)."""
    c, (r64, r32) = d.case, ref
    spec = spec_of(c)
    flat0, Xs = O.flatten(d.params).cuda(), [d.X.cuda()] + ([d.X2.cuda()] if iterations == 2 else [])
    T = None if d.T is None else d.T.cuda()
    scale, cs = torch.tensor(c.term_scale(), device="cuda"), torch.tensor(c.col_scale(), device="cuda")
    nP, nc = flat0.numel(), len(c.fid_cols)
    n_res = c.n_res if c.kind == "split" else (-1 if nc else c.N)
    ran, worst = [], 0.0
    for tag in tags:
        eng, what = Engine(desc_of(c, tag)), f"{c.tag()} / {tag}"
        th, grad, m, v = flat0.clone(), torch.randn(nP, device="cuda"), torch.zeros(nP, device="cuda"), torch.zeros(nP, device="cuda")
        base, ts, csm = grad.clone(), poisoned(spec.n_terms), poisoned(nc)
        kw = dict(T=T, out_col=c.fid_cols, col_scale=cs if nc else None, term_sums=ts, col_sums=csm if nc else None)
        try:
            folded = eng.loss_grad_adam_step(spec, scale, th, Xs[0], n_res, grad, m, v, 1, c.lr, **kw)
        except PinnError as err:          # (an engine the shape has no workspace for: refused before the entry)
            assert not K.served("adam", c, tag), (what, err)
            folded = False
        torch.cuda.synchronize()
        assert folded == (K.served("adam", c, tag) and K.adam_folded(c, tag)), (what, folded)
        if not folded:                    # nothing launched, nothing written
            assert torch.equal(th, flat0) and torch.equal(grad, base) and bool((ts == POISON).all()) and bool((m == 0).all()), what
            continue
        worst = max(worst, check_sums(ts, r64.sums, r32.sums, what + " term sums"), check_sums(csm, r64.cols, r32.cols, what + " column sums"),
                    gradient_ratio(grad, r64, r32, c.layers, what + " first gradient"))
        if iterations == 2:
            th1 = O.unflatten(th.cpu().clone(), c.layers)
            # a condition on the case, checked where it can be: the second point set is off the kink of the DEVICE's parameters
            assert bool(K.off_the_kink(th1, d.kink.tau1, d.X2).all()), f"{what}: the second point set sits on the kink of the device's parameters"
            assert eng.loss_grad_adam_step(spec, scale, th, Xs[1], n_res, grad, m, v, 2, c.lr, **kw)
            torch.cuda.synchronize()
            b64, b32 = (K.evaluate(c, th1, d.X2, d.T, t) for t in (torch.float64, torch.float32))
            worst = max(worst, check_sums(ts, b64.sums, b32.sums, what + " second term sums"),
                        gradient_ratio(grad, b64, b32, c.layers, what + " second gradient"))
        want = O.flatten(K.adam_steps_fp64(c, d.params, [d.X] + ([d.X2] if iterations == 2 else []), d.T))
        got, th0 = th.cpu().double(), flat0.cpu().double()
        dmax, drel = float((got - want).abs().max()), float((got - want).norm() / (want - th0).norm())
        assert dmax < 1.025 * iterations * c.lr and drel < 2e-2, (what, dmax / c.lr, drel)
        ran.append(tag)
    return ran, worst


CHECKS = {"loss": check_loss, "adam": check_adam, "adj": check_adj, "fields": check_fields_entry, "fwd": check_fwd, "second": check_second}


def run_seed(family, seed):
    d = K.data(family, seed)
    ran, worst = CHECKS[family](d, K.reference(family, seed), K.engines(family, d.case))
    print(f"{d.case.tag()}: {'/'.join(ran)} (worst error / bound {worst:.2f})")


# ---- the seeded families -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", K.SEEDS["loss"])
def test_loss_and_gradient(seed):
    """residual_loss, residual_loss_grad, residual_mse_loss_grad, residual_mse_split_loss_grad, mse_loss_grad on GENERIC,
    FUSED_TILE, FUSED_COOP (padded width 64; FUSED_BATCH below it, which has no LeakyReLU instance and falls back to the
    tile kernel) and AUTO."""
    run_seed("loss", seed)


@pytest.mark.parametrize("seed", K.SEEDS["adam"])
def test_two_folded_adam_iterations(seed):
    run_seed("adam", seed)


@pytest.mark.parametrize("seed", K.SEEDS["adj"])
def test_jet_backward(seed):
    run_seed("adj", seed)


@pytest.mark.parametrize("seed", K.SEEDS["fields"])
def test_residual_fields(seed):
    run_seed("fields", seed)


@pytest.mark.parametrize("seed", K.SEEDS["fwd"])
def test_forward_and_jet(seed):
    run_seed("fwd", seed)


@pytest.mark.parametrize("seed", K.SEEDS["second"])
def test_second_order(seed):
    run_seed("second", seed)


def test_plain_forward_at_150001_points():
    """pinn_forward of a 3 x 16 network at 150 001 points: the four-tiles-per-wave plain-forward kernel (k_fused_plain4) under
    AUTO and FUSED; forward only, the fp64 reference is one matrix chain."""
    c = K.Case("fwd", 0, None, 0.0, ("in0", "in1"), ("out0", "out1", "out2"), (), 3, 16, 150001)
    g = torch.Generator().manual_seed(150001)
    params = K._params(c, g)
    Xc, kink = K.kink_free_points(params, c.N, K.sampler_of(c), g)
    assert kink.rejected <= K.MAX_REJECTED
    ref = [O.mlp_forward([p.double() for p in params], Xc.double(), K.INIT)]
    flat, X = O.flatten(params).cuda(), Xc.cuda()
    worst = 0.0
    for tag in ("auto", "fused", "generic"):
        Y = Engine(desc_of(c, tag)).forward(flat, X)
        torch.cuda.synchronize()
        worst = max(worst, check_jets([Y], ref, f"{c.tag()} / {tag}"))
    print(f"{c.tag()}: auto/fused/generic (worst error / bound {worst:.2f}, {100 * kink.rejected:.2f} % of the candidates rejected)")


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", K.SEEDS["loss"][:12])
def test_wide_engine_and_bf16_refuse_leaky_relu(seed):
    """ENGINE_WIDE (wide_supports requires tanh) and bf16 precision (the wide engine only) refuse every LeakyReLU loss and
    forward request at any width, before any device work: pre-filled outputs stay as they were."""
    d = K.data("loss", seed)
    c = d.case
    spec = spec_of(c)
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    T = None if d.T is None else d.T.cuda()
    scale = torch.tensor(c.term_scale(), device="cuda") if c.res else None
    cs = torch.tensor(c.col_scale(), device="cuda")
    for what, desc in (("wide", desc_of(c, "wide")), ("bf16", desc_of(c, "auto", precision=PREC_BF16))):
        eng = Engine(desc)
        grad = torch.randn(flat.numel(), device="cuda")
        base, ts, csm = grad.clone(), poisoned(K.N_TERMS[c.res] if c.res else 0), poisoned(len(c.fid_cols))
        with pytest.raises(PinnError):
            loss_call(eng, c, spec, scale, cs, flat, X, T, grad, ts, csm)
        with pytest.raises(PinnError):
            eng.forward(flat, X)
        torch.cuda.synchronize()
        assert torch.equal(grad, base) and bool((ts == POISON).all()) and bool((csm == POISON).all()), (c.tag(), what)
    print(f"{c.tag()}: ENGINE_WIDE and bf16 refused, nothing written")


# ---- elsewhere: the families without a LeakyReLU instance on the fused engine ---------------------------------------------------
# name: {engine: whether include/pinn_hip.h serves the LeakyReLU request there}, the word its refusals carry
ELSEWHERE = {
    # coefficients / point weights: "FUSED and FUSED_TILE ... tanh"; AUTO "the tile instances where FUSED is served, else GENERIC"
    "coefficient": ({"tile": False, "auto": True, "generic": True}, "LeakyReLU"),
    "weighted": ({"tile": False, "auto": True, "generic": True}, "LeakyReLU"),
    # corrected stress, loss entries: "runs on the engine the descriptor selects, or is refused ... never moved to another engine
    # ... LeakyReLU and k = 3 on FUSED are refused (use GENERIC)": AUTO at width <= 64 selects the fused engine
    "corrected": ({"tile": False, "auto": False, "generic": True}, "corrected"),
    # ensembles: "refused: GENERIC, WIDE, FUSED_COOP, FUSED_BATCH, bf16, LeakyReLU, ..."
    "ensemble": ({"tile": False, "auto": False, "generic": False}, ""),
    # dropout: "gradient passes of tanh networks of hidden width 33..64 run on the fused tile kernel's dropout instances; every
    # other call with dropout_p > 0 runs on the generic engine.  AUTO picks accordingly; FUSED is refused"
    "dropout": ({"tile": False, "auto": True, "generic": True}, "dropout"),
}


@pytest.mark.parametrize("name", sorted(ELSEWHERE))
def test_elsewhere(name):
    """Coefficients, point weights, the corrected radiation stress, ensembles and dropout have no LeakyReLU instance on the
    fused engine: refused there with nothing written, and held to fp64 on the engine the header sends them to."""
    d = K.elsewhere(name)
    c, (r64, r32) = d.case, d.ref
    spec, (rule, word) = spec_of(c), ELSEWHERE[name]
    flat, X = O.flatten(d.params).cuda(), d.X.cuda()
    scale = torch.tensor(c.term_scale(), device="cuda")
    ran, worst = [], 0.0
    for tag, ok in rule.items():
        eng = Engine(desc_of(c, tag, dropout_p=K.DROPOUT_P if name == "dropout" else 0.0))
        eng.dropout_seed = K.DROPOUT_SEED
        what = f"{c.tag()} / {tag}"
        shape = (2, flat.numel()) if name == "ensemble" else (flat.numel(),)
        grad = torch.zeros(shape, device="cuda") if ok else torch.randn(shape, device="cuda")
        base, ts = grad.clone(), poisoned(2 * spec.n_terms if name == "ensemble" else spec.n_terms)
        try:
            if name == "coefficient":
                eng.residual_coef_loss_grad(spec, torch.tensor(spec.coef_defaults, device="cuda"), scale, flat, X, grad=grad, sums=ts)
            elif name == "weighted":
                eng.residual_weighted_loss_grad(spec, d.kw["weights"].cuda(), scale, flat, X, grad=grad, sums=ts)
            elif name == "ensemble":
                why = eng.ensemble_refusal(spec, 2, c.N, c.N, 0)
                assert why is not None and (tag == "generic" or "LeakyReLU" in why), (what, why)
                eng.ensemble_loss_grad(spec, scale, torch.stack([flat, flat]), X, c.N, grad, term_sums=ts.view(2, -1))
            else:
                eng.residual_loss_grad(spec, scale, flat, X, grad, sums=ts)
        except PinnError as err:
            assert not ok, f"{what}: refused although include/pinn_hip.h documents it as served: {err}"
            assert word in str(err), (what, str(err))
            torch.cuda.synchronize()
            assert torch.equal(grad, base) and bool((ts == POISON).all()), f"{what}: a refused call wrote to its outputs"
            continue
        assert ok, f"{what}: served although include/pinn_hip.h documents it as refused"
        torch.cuda.synchronize()
        worst = max(worst, check_sums(ts, r64.sums, r32.sums, what + " term sums"), gradient_ratio(grad, r64, r32, c.layers, what))
        ran.append(tag)
    print(f"{c.tag()}: {'/'.join(ran) or 'refused everywhere'} (worst error / bound {worst:.2f})")


# ---- the named cases on the kink ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,W,k", K.NAMED)
def test_on_the_kink(name, L, W, k):
    """origin: z == 0.0 in every unit of every layer at one grid point; axis: exact zeros in half of the first layer's units on
    the rows of one grid plane.  Exact arithmetic on both sides: the slope there is 0.01, forward and reverse."""
    lines = []
    for family in ("loss", "adj", "fields", "fwd", "second"):
        d = K.named(name, L, W, k, family)
        ran, worst = CHECKS[family](d, K.named_reference(name, L, W, k, family), K.engines(family, d.case))
        lines.append(f"{family} {'/'.join(ran)} {worst:.2f}")
    d = K.named(name, L, W, k, "loss")
    ran, worst = check_adam(d, K.named_reference(name, L, W, k, "loss"), ["auto", "tile"], iterations=1)
    lines.append(f"adam (one iteration) {'/'.join(ran)} {worst:.2f}")
    print(f"{name} {L}x{W} k={k} ({d.case.N} points, {d.kink.exact_zeros} exact zeros): " + "; ".join(lines))


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name,L,W,k", [n for n in K.NAMED if n[0] == "origin"])
def test_negative_zero_gives_the_bits_of_positive_zero(name, L, W, k):
    """The origin case with every 0.0 of X replaced by -0.0: z is -0.0 or +0.0, never > 0, and every output must carry the
    bits of the +0.0 run (the point sets are two tiles: one workgroup adds them in either order to the same sum)."""
    out = {}
    for neg in (False, True):
        res = []
        for family in ("loss", "adj", "fields", "fwd"):
            d = K.named(name, L, W, k, family, negative_zero=neg)
            c = d.case
            assert bool(((d.X == 0) & (torch.signbit(d.X) == neg)).any())
            flat, X = O.flatten(d.params).cuda(), d.X.cuda()
            for tag in ("tile", "generic"):
                eng = Engine(desc_of(c, tag))
                if family == "fwd":
                    res += [eng.forward(flat, X), *eng.forward_jet(flat, X)]
                elif family == "fields":
                    res.append(eng.residual_fields(spec_of(c), flat, X))
                elif family == "adj":
                    grad = torch.zeros(flat.numel(), device="cuda")
                    res.append(eng.jet_backward(flat, X, d.gY.cuda(), d.gdY.cuda(), grad))
                else:
                    grad = torch.zeros(flat.numel(), device="cuda")
                    res += [eng.residual_loss_grad(spec_of(c), torch.tensor(c.term_scale(), device="cuda"), flat, X, grad), grad]
        torch.cuda.synchronize()
        out[neg] = res
    for i, (a, b) in enumerate(zip(out[False], out[True])):
        assert torch.equal(bits(a), bits(b)), (name, L, W, k, i, float((a - b).abs().max()))
    print(f"{name} {L}x{W} k={k}: {len(out[True])} outputs bit-identical under X = -0.0")

"""bf16 mode of the wide engine (the chain kernels of csrc/chain_kernel.h, k_chain_pack and the bf16 branch of run_w) against
the fp64 rounding model of tests/chain_model_util.py: term sums, fidelity sums, EVERY gradient block and the per-point jets,
each within max(the project's fp32 floor, 4 x the case's emulation noise) — a bound computed from the case, at most 1e-3 on
every sum and block (tests/test_chain_model_cpu.py holds the cases to that), where the exact-arithmetic tests of bf16 mode
need 5e-3 .. 1e-1.

The cases: a fixed table (depth 1 .. 4 and a damped depth 6; widths 65 .. 256 in both translation units; K1 = 1, 3, 4; the
folded and the wide first layer; k_chain_last_bwd and the wide output layer; point counts 1, 15, 16, 17, 70 and around the
batch size B = 64 x CUs up to beyond 8 B, read from the device), a seeded sweep, the same points in a permuted order, and
repeated calls on one engine and workspace.  No case is skipped because kernel and model disagree; a sweep draw only for a
condition of its reference (listed by seed by the CPU module).

Measured on an MI355X (256 CUs; the module takes 27 s, its slowest test 2.3 s), worst distance / bound per family:
  table, up to 4 000 points              0.29  (L3_ns_w129_n70, W3)
  table, B - 1 .. 8 B + 33 points        0.25  (L3_ns_w100_2Bp17_mse, a fidelity sum)
  sweep, 39 draws (7022 skipped: its reference's bounds reach 9.5e-3 at ONE point, above the 1e-3 cap)
                                         0.33  (seed 7013, NS 3 x 129, 243 points)
  permuted points                        Y and dY bit-equal at every point, term sums equal, gradient blocks 5e-7
  repeated calls on one workspace        0.22  (the smaller call after the larger one, Y2)

The first run, whose emulations all used correctly rounded exp and reciprocal, missed two bounds narrowly: sweep 7015 (NS 4 x 72,
split request, 16 383 points) had W2, W3, W4 at 1.03, 1.09, 1.16 of 3.7e-5 .. 3.0e-5, and L2_ns4_w256_n37 one term sum at 1.06
of 2.4e-5.  The cause is no defect of the kernels: v_exp_f32 and v_rcp_f32 are accurate to 1 ulp and a one-sided error does not
average out over the points; emulations with both results one ulp off are part of the noise now, the rule
max(floor, 4 x noise) is as it was.
"""
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import ENGINE_WIDE, PREC_BF16
from tests import chain_model_util as M

pytestmark = pytest.mark.gpu


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def engine(c):
    return Engine(NetDesc(c.d_in, c.d_out, c.L, c.W, c.gc, engine=ENGINE_WIDE, precision=PREC_BF16))


def call(eng, c, kind, params, X, T, rq, grad=None):
    """One call of `kind` on the engine: the result in the model's terms (chain_model_util.run)."""
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    spec = ResidualSpec.from_names(c.res, c.inn, c.gc, c.outn)
    cols, sc, cs = list(rq["cols"]), rq["scale"].cuda(), rq["cscale"].cuda()
    if grad is None:
        grad = torch.zeros(eng.n_params, device="cuda")
    out = {}
    if kind == "residual":
        out["sums"] = eng.residual_loss_grad(spec, sc, flat, Xd, grad)
    elif kind == "mse":
        out["csums"] = eng.mse_loss_grad(flat, Xd, T.cuda().contiguous(), cols, cs, grad)
    elif kind == "split":
        Tf = T[: X.shape[0] - rq["n_res"]].cuda().contiguous()
        out["sums"], out["csums"] = eng.residual_mse_split_loss_grad(spec, sc, Tf, cols, cs, flat, Xd, rq["n_res"], grad)
    elif kind == "onepass":
        out["sums"], out["csums"] = eng.residual_mse_loss_grad(spec, sc, T.cuda().contiguous(), cols, cs, flat, Xd, grad)
    elif kind == "forward":
        out["Y"] = eng.forward(flat, Xd)
    elif kind == "jet":
        out["Y"], out["dY"] = eng.forward_jet(flat, Xd)
    elif kind == "fields":
        out["fields"] = eng.residual_fields(spec, flat, Xd)
    if kind in ("residual", "mse", "split", "onepass"):
        out["grad"] = grad
    torch.cuda.synchronize()
    return {k: v.detach().double().cpu() for k, v in out.items()}


def check(c, kind, got, what):
    model, bound, _ = M.reference(c, kind, cus())
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (what, k)
    r = M.ratios(c, got, model, bound)
    assert r, what
    k = max(r, key=r.get)
    print(f"CHAIN GPU | {what} {kind} N={c.N(cus())}: worst distance / bound {r[k]:.2f} in {k} (bound {bound[k]:.1e}; "
          f"{len(r)} quantities)")
    bad = {q: f"{v:.2f} x {bound[q]:.1e}" for q, v in r.items() if not v <= 1.0}
    assert not bad, (what, kind, bad)
    return r[k]


@pytest.mark.parametrize("c", M.TABLE, ids=lambda c: c.name)
def test_table_case_against_the_rounding_model(c):
    params, X, T = c.data(cus())
    eng = engine(c)
    for kind in c.calls:
        check(c, kind, call(eng, c, kind, params, X, T, c.request(kind, cus())), c.name)


@pytest.mark.parametrize("seed", M.SWEEP_SEEDS)
def test_sweep_draw_against_the_rounding_model(seed):
    c = M.draw(seed)
    kind = c.calls[0]
    why = M.cancelling(c, kind, cus())
    if why is None and M.capped(c, M.reference(c, kind, cus())[1]):
        why = "bound above the 1e-3 cap"
    if why:
        pytest.skip(f"seed {seed}: {why} (a condition of the reference; tests/test_chain_model_cpu.py lists the seeds)")
    params, X, T = c.data(cus())
    check(c, kind, call(engine(c), c, kind, params, X, T, c.request(kind, cus())),
          f"seed {seed} {c.net} {c.L}x{c.W} gain {c.gain}")


PERMUTED = [M.Case("perm_L3_ns_w65_Bp83", "ns", 3, 65, (1, 83)), M.Case("perm_L2_cf_w256_n1000", "cf", 2, 256, (0, 1000)),
            M.Case("perm_L2_ns4_w100_n243", "ns4", 2, 100, (0, 243))]


@pytest.mark.parametrize("c", PERMUTED, ids=lambda c: c.name)
def test_permuted_points(c):
    """The same points in another order land in other tiles, waves, workgroups and batches.  A point's jet is computed from
    its own MFMA column, its own lanes' activation and the shared weights only (chain_kernel.h: the waves of a tile are
    independent, act() and make_a1() are lane-local up to the point's own two lanes), so forward_jet must return the SAME
    BITS per point; sums and gradients change their summation order and stay within the fp32 floor."""
    params, X, T = c.data(cus())
    rq = c.request("residual", cus())
    perm = torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(5))
    eng = engine(c)
    a = call(eng, c, "jet", params, X, T, rq)
    b = call(eng, c, "jet", params, X[perm].contiguous(), T, rq)
    dy = int((b["Y"] != a["Y"][perm]).sum()), int((b["dY"] != a["dY"][:, perm]).sum())
    ga = call(eng, c, "residual", params, X, T, rq)
    gb = call(eng, c, "residual", params, X[perm].contiguous(), T, rq)
    es = float(((gb["sums"] - ga["sums"]).abs() / ga["sums"].abs().clamp_min(1e-300)).max())
    eb = M.distances(c, dict(grad=gb["grad"]), dict(grad=ga["grad"]))
    print(f"CHAIN GPU | {c.name}: {dy[0]} / {dy[1]} differing Y / dY entries, sums {es:.1e}, worst block {max(eb.values()):.1e}")
    assert dy == (0, 0), dy
    assert es < M.FLOOR["sum"] and max(eb.values()) < M.FLOOR["block"], (es, eb)


def test_repeated_calls_on_one_workspace():
    """A smaller call after a larger one on the same engine and workspace, then the same small set laid over two calls that
    accumulate into one gradient: nothing of the earlier calls' jets may be read."""
    big = M.Case("rep_L3_ns_w65_Bp83", "ns", 3, 65, (1, 83))
    small = M.Case("rep_L3_ns_w65_n1000", "ns", 3, 65, (0, 1000))
    eng = engine(big)
    pb, Xb, Tb = big.data(cus())
    check(big, "residual", call(eng, big, "residual", pb, Xb, Tb, big.request("residual", cus())), big.name)
    ws = eng.workspace(Xb.shape[0])
    ps, Xs, Ts = small.data(cus())
    assert all(bool((a == b).all()) for a, b in zip(pb, ps))
    rq = small.request("residual", cus())
    check(small, "residual", call(eng, small, "residual", ps, Xs, Ts, rq), small.name + " after the larger call")
    check(small, "jet", call(eng, small, "jet", ps, Xs, Ts, rq), small.name + " after the larger call")
    assert eng.workspace(Xs.shape[0]).data_ptr() == ws.data_ptr()
    grad = torch.zeros(eng.n_params, device="cuda")
    n1 = 333
    one = call(eng, small, "residual", ps, Xs[:n1], Ts, rq, grad=grad)
    two = call(eng, small, "residual", ps, Xs[n1:], Ts, rq, grad=grad)
    check(small, "residual", dict(sums=one["sums"] + two["sums"], grad=two["grad"]), small.name + " laid over two calls")

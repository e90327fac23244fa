"""The hand-written device math (tanh_f32, tanh_f32x2, tanh_bf, sincos_f64arg, sin_layer_z, to_bf16x4 / from_bf16x4) held to
its own comments over ALL fp32 bit patterns, through the test-only probe library (csrc/pinn_probe.hip), and tied to what
the product kernels compute.

Every bound asserted here is a claim in the source, a bound derived in the test's docstring, or bitwise equality.  The
reference of the scans is the device library's fp64 tanh / sin / cos, which the first test holds to the host's libm."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import devmath_util as D

pytestmark = pytest.mark.gpu

ALL = 1 << 32
FINITE = D.binade_rows(0, 254)


@functools.lru_cache(maxsize=None)
def scan(fn: int) -> np.ndarray:
    t = D.probe_scan_all(fn)
    t.setflags(write=False)
    return t


def _viol(t, j, rows=None) -> int:
    return int((t if rows is None else t[rows])[:, D.S_VIOL + j].sum())


def _where(bits: int) -> str:
    return f"{float(D.f32_of([bits])[0])!r} ({bits:#010x})"


def _per_binade(t, slot, rows, what):
    for r in rows:
        if t[r, D.S_COUNT]:
            v = float(t[r:r + 1, slot].view(np.float64)[0])
            print(f"  {what} binade 2^{(int(r) & 255) - 127:+d}{' (-)' if r >= 256 else ''}: {v:.3e} at {_where(int(t[r, slot + 1]))}")


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_device_fp64_reference_against_libm():
    """The device library's double tanh, sin, cos within 4 ulp of fp64 of the host libm's on 2^20 log-spaced inputs of both
    signs plus the special values (tanh's inputs are fp32 values: that is how the scans call it)."""
    n = 1 << 19
    mag32 = np.exp(np.linspace(math.log(1e-45), math.log(3e38), n)).astype(np.float32)
    x32 = np.concatenate([mag32, -mag32, np.array([0.0, -0.0, 0.625, -0.625, 1.0, 20.0, np.inf, -np.inf], np.float32)])
    got = D.probe_ref(D.FN_TANH_F32, x32)
    ref = np.array([math.tanh(v) for v in x32.astype(np.float64)])
    u = np.abs(got - ref) / D.ulp64(ref)
    print(f"device fp64 tanh vs libm: max {u.max():.2f} ulp at {x32[int(np.argmax(u))]!r}")
    assert u.max() <= 4 and np.array_equal(np.signbit(got), np.signbit(ref))
    assert np.isnan(D.probe_ref(D.FN_TANH_F32, np.array([np.nan], np.float32))[0])

    mag = np.exp(np.linspace(math.log(1e-300), math.log(2.0 ** 31), n))
    k = np.arange(1, 1025, dtype=np.float64)
    z = np.concatenate([mag, -mag, k * (np.pi / 2), -k * (np.pi / 2), np.array([0.0, -0.0, np.pi / 4, 1024.0, 65536.0])])
    got = D.probe_ref(D.FN_SINCOS, z)
    for c, f, name in ((0, math.sin, "sin"), (1, math.cos, "cos")):
        ref = np.array([f(v) for v in z])
        u = np.abs(got[:, c] - ref) / D.ulp64(ref)
        print(f"device fp64 {name} vs libm: max {u.max():.2f} ulp at {z[int(np.argmax(u))]!r}")
        assert u.max() <= 4
    bad = D.probe_ref(D.FN_SINCOS, np.array([np.nan, np.inf, -np.inf]))
    assert np.all(np.isnan(bad))


# ---- tanh_f32 -----------------------------------------------------------------------------------------------------------------
def test_tanh_f32_scan():
    """residuals.h::tanh_f32 at all 2^32 patterns: 'abs error <= ~1.5e-7 everywhere' for every finite input, 'relative error
    ~1e-7' (asserted: 1.0e-7) for 0 < |x| < 0.625 with the subnormals, and the invariants every caller leans on:
    tanh(-x) = -tanh(x) bitwise, |a| <= 1 (so that s = 1 - a^2 >= 0), +-0 -> +-0, +-inf -> +-1, NaN -> NaN."""
    t = scan(D.FN_TANH_F32)
    assert int(t[:, D.S_COUNT].sum()) == ALL
    e_abs, at_abs = D.worst(t, D.S_ABS, FINITE)
    e_rel, at_rel = D.worst(t, D.S_REL, FINITE)
    back, at_back = D.worst(t, D.S_AUX, FINITE)
    print(f"tanh_f32: max abs error {e_abs:.4e} at {_where(at_abs)}; max relative error below 0.625 {e_rel:.4e} at {_where(at_rel)}; "
          f"largest backward step between neighbouring patterns {back:.3e} at {_where(at_back)}")
    names = {D.V_ODD: "tanh(-x) != -tanh(x)", D.V_RANGE: "|a| > 1", D.V_ZERO: "+-0 -> +-0", D.V_INF: "+-inf -> +-1", D.V_NAN: "NaN -> NaN"}
    broken = {names[j]: _viol(t, j) for j in names if _viol(t, j)}
    assert not broken, broken
    assert e_abs <= 1.5e-7
    assert e_rel <= 1.0e-7
    assert int(t[D.binade_rows(255, 255), D.S_COUNT].sum()) == 1 << 24        # the inf / NaN rows were visited too


def test_tanh_f32_polynomial_is_the_cpu_model():
    """Below 0.625 the device result is the numpy restatement bit for bit (multiply and fma only; test_devmath_cpu.py holds
    that restatement to fp64): 2^20 sampled patterns of both signs, subnormals and the patterns next to the switch included."""
    rng = np.random.default_rng(17)
    top = int(D.bits_of([0.625])[0])
    mag = np.concatenate([rng.integers(0, top, (1 << 19) - 4096, dtype=np.int64), rng.integers(0, 1 << 23, 2048, dtype=np.int64),
                          np.arange(top - 2048, top, dtype=np.int64)]).astype(np.uint32)
    bits = np.concatenate([mag, mag | np.uint32(0x80000000)])
    got = D.probe_eval(D.FN_TANH_F32, bits)
    model = D.tanh_f32_model(D.f32_of(bits))
    nz = (bits & np.uint32(0x7fffffff)) != 0            # (a zero's sign is tanh_f32's final copysign, not the polynomial's)
    assert np.array_equal(D.bits_of(got)[nz], D.bits_of(model)[nz])
    assert np.array_equal(D.bits_of(got)[~nz], bits[~nz])
    # the switch itself: the 8 patterns on either side run on different branches and both keep the absolute bound
    sw = np.arange(top - 8, top + 8, dtype=np.uint32)
    y = D.probe_eval(D.FN_TANH_F32, sw).astype(np.float64)
    assert np.max(np.abs(y - np.tanh(D.f32_of(sw).astype(np.float64)))) <= 1.5e-7


def test_tanh_f32x2_scan():
    """'each half is bitwise tanh_f32 of its input': all 2^32 patterns through the first half, and through the second half in
    bit-reversed order; NaN compared as NaN; no mismatch allowed."""
    t = scan(D.FN_TANH_F32X2)
    assert int(t[:, D.S_COUNT].sum()) == ALL and int(t[:, D.S_COUNT2].sum()) == ALL
    assert (_viol(t, 0), _viol(t, 1)) == (0, 0)
    x = np.array([0.0, -0.0, 0.3, -0.3, 0.625, -0.625, 5.0, -5.0, np.inf, -np.inf, 1e-40, 100.0], np.float32)
    both = D.probe_eval(D.FN_TANH_F32X2, x)
    one = D.probe_eval(D.FN_TANH_F32, x)
    assert np.array_equal(D.bits_of(both[0]), D.bits_of(one)) and np.array_equal(D.bits_of(both[1]), D.bits_of(one[::-1]))


# ---- tanh_bf ------------------------------------------------------------------------------------------------------------------
def test_tanh_bf_scan():
    """chain_kernel.h::tanh_bf(x) = fma(-2, rcp(e + 1), 1), e = __expf(2x) = exp2(fl(2x * log2e_f32)), at all 2^32 patterns.

    The bound, from the expression's own roundings, with u = exp(2x) the exact exponential (one ulp is at most 2^-23 relative):
      * 2x is exact; t = fl(2x * log2e_f32) has relative error 2^-24 from the product plus d_c = |log2e_f32 - log2 e| / log2 e
        (1.3e-8) from the constant; an error dt of the argument of exp2 is a relative error ln2 * dt of its value, and
        ln2 * |t| = |2x|: (2^-24 + d_c) |2x|.  The hardware exp2 adds one ulp:   eps_e = 2^-23 + |2x| (2^-24 + d_c)
      * d = fl(e + 1): the error of e enters with weight u / (u + 1), the sum rounds once (2^-24), the hardware reciprocal adds
        one ulp (the source's own assumption):                                 eps_r = eps_e u / (u + 1) + 2^-24 + 2^-23
      * the result 1 - 2 r is ONE fma: the error of r enters as 2 r eps_r = 2 / (u + 1) eps_r, and the rounding of a result
        of magnitude below 1 is at most 2^-25.
    |error| <= sup_x [ 2 / (u + 1) * eps_r ] + 2^-25 = 4.0e-7 (devmath_util.tanh_bf_bound), reached on the negative side, where
    2 / (u + 1) lies in (1, 2): there the result is near -1 and carries twice the reciprocal's error.
    Measured maximum: see DESIGN.md 4.6 and the comment in chain_kernel.h."""
    t = scan(D.FN_TANH_BF)
    assert int(t[:, D.S_COUNT].sum()) == ALL
    bound = D.tanh_bf_bound()
    e_abs, at_abs = D.worst(t, D.S_ABS, FINITE)
    e_pos, at_pos = D.worst(t, D.S_ABS, np.arange(0, 255))
    e_rel, at_rel = D.worst(t, D.S_REL, FINITE)
    print(f"tanh_bf: max abs error {e_abs:.4e} at {_where(at_abs)} (x > 0: {e_pos:.4e} at {_where(at_pos)}); derived bound {bound:.4e}; "
          f"max relative error {e_rel:.3e} at {_where(at_rel)}")
    assert (_viol(t, D.V_RANGE), _viol(t, D.V_INF), _viol(t, D.V_NAN)) == (0, 0, 0)
    assert e_abs <= bound


# ---- sincos_f64arg, sin_layer_z -----------------------------------------------------------------------------------------------
SIN_DOMAIN = D.binade_rows(0, 136)          # every fp32 value with |z| < 1024 (1024 itself: checked with the doubles)


def test_sincos_scan_fp32_arguments():
    """'Absolute error <= 7e-8 for both against fp64': every fp32 value with
    |z| <= 1024 (as the double it converts to).  Up to 2^30 only |sn| <= 1 and |cs| <= 1 are asserted and the error is printed
    per binade; NaN and +-inf give NaN."""
    t = scan(D.FN_SINCOS)
    assert int(t[:, D.S_COUNT].sum()) == ALL
    es, at_s = D.worst(t, D.S_ABS, SIN_DOMAIN)
    ec, at_c = D.worst(t, D.S_AUX, SIN_DOMAIN)
    print(f"sincos_f64arg, |z| < 1024: max abs error sin {es:.4e} at {_where(at_s)}, cos {ec:.4e} at {_where(at_c)}")
    print("beyond the asserted domain (printed, not asserted):")
    _per_binade(t, D.S_ABS, range(137, 255), "sin")
    assert _viol(t, D.V_RANGE, D.binade_rows(0, 156)) == 0        # |z| < 2^30
    assert _viol(t, D.V_NAN) == 0
    assert es <= D.SINCOS_CLAIM and ec <= D.SINCOS_CLAIM


def test_sincos_double_arguments():
    """The same bound where an fp32 argument never lands: doubles within +-2^-30 .. +-2^-10 of k pi/2 for k up to 2^20 (the
    quadrant boundaries of the range reduction, on both sides), 2^22 random doubles with |z| <= 2^16, and |z| = 1024."""
    rng = np.random.default_rng(23)
    k = np.arange(1, (1 << 20) + 1, dtype=np.float64)
    e = 10 + (np.arange(k.size) % 21)                               # every k: one offset, 2^-10 .. 2^-30 in turn, sides alternating
    side = np.where((np.arange(k.size) // 21) % 2 == 0, 1.0, -1.0)
    one = k * (np.pi / 2) + side * np.exp2(-e.astype(np.float64))
    ks = np.arange(1, (1 << 12) + 1, dtype=np.float64)              # the first 2^12 boundaries: every offset on both sides
    every = np.concatenate([ks * (np.pi / 2) + s * 2.0 ** -j for j in range(10, 31) for s in (1.0, -1.0)])
    z = np.concatenate([one, -one, every, -every, k[:4096] * (np.pi / 2), rng.uniform(-65536.0, 65536.0, 1 << 22),
                        np.array([1024.0, -1024.0, 0.0, -0.0, np.pi / 4, -np.pi / 4])])
    got = D.probe_eval(D.FN_SINCOS, z).astype(np.float64)
    ref = D.probe_ref(D.FN_SINCOS, z)
    err = np.abs(got - ref)
    for c, name in ((0, "sin"), (1, "cos")):
        i = int(np.argmax(err[:, c]))
        print(f"sincos_f64arg on doubles: max abs error {name} {err[i, c]:.4e} at z = {z[i]!r}")
    assert np.all(np.abs(got) <= 1.0)
    assert err.max() <= D.SINCOS_CLAIM
    bad = D.probe_eval(D.FN_SINCOS, np.array([np.nan, np.inf, -np.inf]))
    assert np.all(np.isnan(bad))


def test_sincos_is_the_cpu_model():
    """The helper is the numpy restatement bit for bit (every step of it is exact or rounded once; test_devmath_cpu.py holds
    that restatement to fp64 without a GPU): fp32 and double arguments, the quadrant boundaries, both outputs."""
    rng = np.random.default_rng(43)
    k = np.arange(1, 1 << 16, dtype=np.float64)
    z = np.concatenate([rng.uniform(-1024, 1024, 1 << 17).astype(np.float32).astype(np.float64), rng.uniform(-65536.0, 65536.0, 1 << 17),
                        k * (np.pi / 2) + 2.0 ** -20, -k * (np.pi / 2) + 2.0 ** -30, np.array([0.0, -0.0, 1024.0, np.pi / 4])])
    ms, mc = D.sincos_model(z)
    gs = D.probe_eval(D.FN_SINCOS, z)
    assert np.array_equal(D.bits_of(gs[:, 0] + np.float32(0)), D.bits_of(ms + np.float32(0)))
    assert np.array_equal(D.bits_of(gs[:, 1] + np.float32(0)), D.bits_of(mc + np.float32(0)))


def test_sin_layer_z_is_the_fp64_dot_product():
    """z_0 = b + sum_i w[i] x[i] in double for d_in <= 8: the products of fp32 numbers are exact in fp64 and an fma of an
    exact product is the plain rounded sum, so numpy's chain in the same order must give the same bits."""
    rng = np.random.default_rng(29)
    n = 1 << 14
    rec = np.zeros((n, 18), np.float32)
    rec[:, :16] = (rng.standard_normal((n, 16)) * np.exp(rng.uniform(-20, 20, (n, 16)))).astype(np.float32)
    rec[:, 16] = (rng.standard_normal(n) * 100).astype(np.float32)
    rec[:, 17] = np.arange(n) % 9                                    # d_in = 0 .. 8
    got = D.probe_eval(D.FN_SIN_Z, rec)
    ref = rec[:, 16].astype(np.float64)
    for i in range(8):
        ref = np.where(rec[:, 17] > i, ref + rec[:, i].astype(np.float64) * rec[:, 8 + i].astype(np.float64), ref)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------
def test_bf16_conversions_scan():
    """to_bf16x4 ('RNE, NaN-safe') equals the integer round-to-nearest-even at all 2^32 patterns, each in the vector lane its
    low two bits name; a NaN stays a NaN (payload not compared); from_bf16x4 of the result is the pattern shifted up."""
    t = scan(D.FN_TO_BF16)
    assert int(t[:, D.S_COUNT].sum()) == ALL
    assert (_viol(t, 0), _viol(t, 1), _viol(t, D.V_NAN)) == (0, 0, 0)
    # the helper on caller data against the same reference, every lane, and from_bf16x4 on all 2^16 patterns
    rng = np.random.default_rng(31)
    bits = np.concatenate([rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32),
                           np.array([0x7f7fffff, 0xff7fffff, 0x3f808000, 0x3f818000, 0x00008000, 0x7f800000, 0xff800000], np.uint32)])
    bits = bits[~D.is_nan_f32_bits(bits)]
    h = D.probe_eval(D.FN_TO_BF16, bits)
    assert np.array_equal(h, D.bf16_rne_bits(bits)) and np.array_equal(h.astype(np.float64), D.probe_ref(D.FN_TO_BF16, bits))
    nan = D.probe_eval(D.FN_TO_BF16, np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0x7f80ffff], np.uint32))
    assert np.all(D.is_nan_bf16(nan))
    h16 = np.arange(1 << 16, dtype=np.uint32)
    assert np.array_equal(D.bits_of(D.probe_eval(D.FN_FROM_BF16, h16)), h16 << 16)


# ---- the probe and the kernels compute the same thing -------------------------------------------------------------------------
def _tie_inputs() -> np.ndarray:
    """2^16-odd fp32 inputs: 128 patterns in every binade of both signs (first, last and random mantissas; exponent 0 = the
    subnormals), the 8 patterns on either side of tanh_f32's switch, +-0."""
    rng = np.random.default_rng(37)
    man = np.concatenate([np.array([0, 1, (1 << 23) - 1, 1 << 22], np.uint32), rng.integers(0, 1 << 23, 124, dtype=np.int64).astype(np.uint32)])
    mag = ((np.arange(255, dtype=np.uint32) << 23)[:, None] | man[None, :]).reshape(-1)
    top = int(D.bits_of([0.625])[0])
    mag = np.concatenate([mag, np.arange(top - 8, top + 8, dtype=np.uint32)])
    return np.concatenate([mag, mag | np.uint32(0x80000000)])


def _one_unit_params(desc, w_first=1.0, w_mid=1.0, w_last=1.0) -> torch.Tensor:
    """Flat parameters of a network whose only non-zero weights are [0, 0] of every matrix, biases 0: every sum adds exact
    zeros, so the output is the chain of activations of w * x."""
    from oracle import pinn_oracle as O
    ls = desc.layers
    ps = []
    for i in range(len(ls) - 1):
        w = torch.zeros(ls[i + 1], ls[i])
        w[0, 0] = w_first if i == 0 else (w_last if i == len(ls) - 2 else w_mid)
        ps += [w, torch.zeros(ls[i + 1])]
    return O.flatten(ps).cuda()


def _tanh_cases():
    from pinn_depthestimation_amd import _lib as L
    return [("generic", L.ENGINE_GENERIC, 3), ("tile", L.ENGINE_FUSED_TILE, 3), ("auto", L.ENGINE_AUTO, 3), ("wide", L.ENGINE_WIDE, 128)]


@pytest.mark.parametrize("case", ["generic", "tile", "auto", "wide"])
def test_forward_of_one_unit_network_is_tanh_f32(case):
    """d_in = 1, one hidden layer (width 3; the wide engine: 128, one live unit), d_out = 1, W_0 = (1, 0, ..)^T, W_1 = (1, 0, ..),
    biases 0: pinn_forward must return the probe's tanh_f32(x) bit for bit on every engine — the instances, compiled under
    their own flags, compute what the header was measured to compute.  (+-0: z = 1 * x + 0 is +0 for both, IEEE.)
    +-inf: this construction has zero weights on REAL units, and 0 * inf = NaN there in the oracle, so each engine is held to
    what include/pinn_hip.h documents for it: GENERIC and WIDE return NaN as the oracle does; the tile kernel and the plain
    forward kernel read an infinite input as +-FLT_MAX (finite_input), 0 * FLT_MAX = 0, and return tanh_f32(+-FLT_MAX) = +-1."""
    from pinn_depthestimation_amd import Engine, NetDesc
    name, engine, width = next(c for c in _tanh_cases() if c[0] == case)
    bits = np.concatenate([_tie_inputs(), np.array([0, 0x80000000], np.uint32)])
    x = D.f32_of(bits)
    desc = NetDesc(1, 1, 1, width, (), engine=engine)
    Y = Engine(desc, "cuda:0").forward(_one_unit_params(desc), torch.from_numpy(x.copy()).cuda().reshape(-1, 1))
    got = Y.cpu().numpy().reshape(-1)
    want = D.probe_eval(D.FN_TANH_F32, x + np.float32(0))            # the bias add: -0 + 0 = +0
    bad = np.nonzero(D.bits_of(got) != D.bits_of(want))[0]
    assert bad.size == 0, (name, bad.size, [(_where(int(bits[i])), got[i], want[i]) for i in bad[:8]])
    Yi = Engine(desc, "cuda:0").forward(_one_unit_params(desc), torch.tensor([[math.inf], [-math.inf], [0.5]], device="cuda")).cpu().numpy().reshape(-1)
    half = D.probe_eval(D.FN_TANH_F32, np.float32([0.5]))[0]
    if case in ("generic", "wide"):
        assert np.isnan(Yi[0]) and np.isnan(Yi[1]) and Yi[2] == half, (name, Yi)
    else:
        assert np.array_equal(Yi, np.float32([1.0, -1.0, half])), (name, Yi)


@pytest.mark.parametrize("case", ["generic", "tile", "auto"])
def test_forward_of_one_unit_sine_network_is_sincos(case):
    """activation = sine first layer, d_in = 2 (the second input column and its weight are zero: the tile kernel's sine
    instances carry 0, 2 or 3 tangents, not 1), two hidden layers of width 3: Y = W_2 tanh(W_1 sin(x)) with W_1 = 2^-13 and
    W_2 = 2^13 on the one live path.  For |u| <= 2^-13 tanh_f32(u) is u bit for bit (the polynomial's correction u * p u^2 is
    below a quarter ulp of u) and the two scalings are powers of two, so pinn_forward must return the probe's sine of
    sincos_f64arg((double)x) bit for bit; the layer-0 tangent of pinn_forward_jet along x is the cosine the same way
    (s_1 = 1 - a_1^2 rounds to 1), and along the dead column it is zero."""
    from pinn_depthestimation_amd import Engine, NetDesc, _lib as L
    engine = {"generic": L.ENGINE_GENERIC, "tile": L.ENGINE_FUSED_TILE, "auto": L.ENGINE_AUTO}[case]
    rng = np.random.default_rng(41)
    x = np.concatenate([rng.uniform(-1024, 1024, 1 << 15), np.arange(1, 2049) * (np.pi / 2), -np.arange(1, 2049) * (np.pi / 2),
                        np.exp(rng.uniform(math.log(1e-20), math.log(1024.0), 1 << 14)), [0.0, 0.5, -0.5, 1024.0, -1024.0]]).astype(np.float32)
    want = D.probe_eval(D.FN_SINCOS, x.astype(np.float64))
    Xd = torch.zeros(x.size, 2)
    Xd[:, 0] = torch.from_numpy(x.copy())
    Xd = Xd.cuda()
    desc = NetDesc(2, 1, 2, 3, (), activation=L.ACT_SIN_TANH, engine=engine)
    th = _one_unit_params(desc, 1.0, 2.0 ** -13, 2.0 ** 13)
    got = Engine(desc, "cuda:0").forward(th, Xd).cpu().numpy().reshape(-1)
    bad = np.nonzero(D.bits_of(got + np.float32(0)) != D.bits_of(want[:, 0] + np.float32(0)))[0]
    assert bad.size == 0, (case, "sin", bad.size, [(x[i], got[i], want[i, 0]) for i in bad[:8]])
    dj = NetDesc(2, 1, 2, 3, (0, 1), activation=L.ACT_SIN_TANH, engine=engine)
    Yj, dY = Engine(dj, "cuda:0").forward_jet(th, Xd)
    assert np.array_equal(D.bits_of(Yj.cpu().numpy().reshape(-1)), D.bits_of(got))
    gc = dY.cpu().numpy().reshape(2, -1)
    bad = np.nonzero(D.bits_of(gc[0] + np.float32(0)) != D.bits_of(want[:, 1] + np.float32(0)))[0]
    assert bad.size == 0, (case, "cos", bad.size, [(x[i], gc[0, i], want[i, 1]) for i in bad[:8]])
    assert np.all(gc[1] == 0)

"""The numpy restatements of the device math helpers (tests/devmath_util.py), held to fp64 without a GPU.

tests/test_devmath_gpu.py compares the device's tanh_f32 with `tanh_f32_poly` bit for bit and its bf16 conversions with
`bf16_rne_bits`; this module shows that those two references are themselves right: the polynomial (whose steps are multiply
and fma only, so the model IS the device arithmetic) keeps the source's relative-error claim, and the integer rounding is
torch's bfloat16 conversion."""
import numpy as np
import torch

from tests import devmath_util as D


def _patterns(lo: float, hi: float, stride: int) -> np.ndarray:
    a, b = int(D.bits_of([lo])[0]), int(D.bits_of([hi])[0])
    return D.f32_of(np.arange(a, b, stride, dtype=np.uint32))


def test_fma32_is_one_rounding():
    """fma32 against exact rational arithmetic on random operands and on constructed double-rounding traps."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(4000) * 1e-4)).astype(np.float32)   # heavy cancellation
    c[::3] = rng.standard_normal(c[::3].size).astype(np.float32)
    # traps: a * b + c whose fp64 sum lands exactly on an fp32 tie although the exact value does not
    a[:4] = np.float32(1 + 2.0 ** -23); b[:4] = np.float32(1 + 2.0 ** -23)
    c[:4] = np.array([2.0 ** -24, -2.0 ** -24, 2.0 ** 30, -2.0 ** 30], np.float32)
    got = D.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # correctly rounded fp32 of the exact value: via the two neighbouring candidates
        g = float(got[i])
        lo, hi = float(np.nextafter(got[i], np.float32(-np.inf))), float(np.nextafter(got[i], np.float32(np.inf)))
        d = abs(Fraction(g) - exact)
        assert d <= abs(Fraction(lo) - exact) and d <= abs(Fraction(hi) - exact), (i, a[i], b[i], c[i], got[i])
        if d == abs(Fraction(lo) - exact) or d == abs(Fraction(hi) - exact):       # a true tie: the even one
            assert int(D.bits_of([got[i]])[0]) & 1 == 0 or d == 0, (i, got[i])


def test_tanh_poly_relative_error():
    """residuals.h: 'relative error ~1e-7' below 0.625 — asserted at 1.0e-7 on every 7th pattern of [0.25, 0.625), where the
    polynomial's error peaks, on every 1021st pattern of the normal numbers below and on a stride of the subnormals (every
    7th pattern of the whole range measures the same 7.6e-8; the GPU scan visits every pattern)."""
    x = np.concatenate([_patterns(0.25, 0.625, 7), _patterns(2.0 ** -126, 0.25, 1021),
                        D.f32_of(np.arange(1, 1 << 23, 4099, dtype=np.uint32)),
                        D.f32_of(np.array([int(D.bits_of([0.625])[0]) - 1], np.uint32))])
    y = D.tanh_f32_poly(x).astype(np.float64)
    ref = np.tanh(x.astype(np.float64))
    rel = np.abs(y - ref) / ref
    i = int(np.argmax(rel))
    print(f"tanh_f32 polynomial branch: max relative error {rel[i]:.3e} at x = {x[i]!r} over {x.size} patterns")
    assert rel[i] <= 1.0e-7
    # odd; and zero at zero (the sign of a zero is put on by tanh_f32's final copysign, outside the polynomial)
    assert np.array_equal(D.bits_of(D.tanh_f32_poly(-x)), D.bits_of(-D.tanh_f32_poly(x)))
    assert np.all(D.tanh_f32_poly(np.array([0.0, -0.0], np.float32)) == 0)


def test_tanh_exp_branch_with_exact_primitives():
    """The exponential branch with correctly rounded exp and reciprocal keeps the source's 1.5e-7 absolute bound with room:
    what the hardware's one-ulp primitives add on top is what the GPU scan measures (measured here: 7.9e-8; the GPU: 9.7e-8)."""
    x = np.concatenate([_patterns(0.625, 12.0, 61), np.array([0.625, 20.0, 50.0, 100.0, 3e38, np.inf], np.float32)])
    y = D.tanh_f32_exp(x).astype(np.float64)
    ref = np.tanh(x.astype(np.float64))
    err = np.abs(y - ref)
    i = int(np.argmax(err))
    print(f"tanh_f32 exponential branch, exact primitives: max abs error {err[i]:.3e} (relative {np.max(err / ref):.3e}) at x = {x[i]!r}")
    assert err[i] <= 1.5e-7
    assert np.all(np.abs(y) <= 1.0)
    assert np.array_equal(D.bits_of(D.tanh_f32_exp(-x)), D.bits_of(-D.tanh_f32_exp(x)))
    m = D.tanh_f32_model(np.array([0.1, -0.1, 0.7, -0.7, np.inf, -np.inf], np.float32))
    assert np.array_equal(m, np.concatenate([D.tanh_f32_poly(np.float32([0.1, -0.1])), D.tanh_f32_exp(np.float32([0.7, -0.7, np.inf, -np.inf]))]))


def test_sincos_model_keeps_the_claim():
    """residuals.h: 'absolute error <= 7e-8 for both' — the restatement (exact or single-rounded steps only) on fp32 arguments
    up to 1024, on doubles up to 2^16 and next to the quadrant boundaries k pi/2 (measured: 5.4e-8).  Without the two carried
    rounding errors (rl, res) the same restatement measures 9.3e-8: what the helper computed before the claim was tested."""
    rng = np.random.default_rng(11)
    k = np.arange(1, 1 << 14, dtype=np.float64)
    near = np.concatenate([s * (k * (np.pi / 2) + t * 2.0 ** -e) for s in (1, -1) for t in (1, -1) for e in (10, 20, 30)])
    z = np.concatenate([
        rng.uniform(-1024, 1024, 1 << 18).astype(np.float32).astype(np.float64),
        rng.uniform(-65536, 65536, 1 << 18),
        near, np.array([0.0, -0.0, np.pi / 4, -np.pi / 4, 1e-300, 2.0 ** -149])])
    sn, cs = D.sincos_model(z)
    es, ec = np.abs(sn - np.sin(z)), np.abs(cs - np.cos(z))
    print(f"sincos model: max abs error sin {es.max():.3e} at {z[int(np.argmax(es))]!r}, cos {ec.max():.3e} at {z[int(np.argmax(ec))]!r}")
    assert es.max() <= D.SINCOS_CLAIM and ec.max() <= D.SINCOS_CLAIM
    assert np.all(np.abs(sn) <= 1) and np.all(np.abs(cs) <= 1)
    with np.errstate(all="ignore"):
        sn, cs = D.sincos_model(np.array([np.nan, np.inf, -np.inf]))
    assert np.all(np.isnan(sn)) and np.all(np.isnan(cs))


def _torch_bf16_bits(bits: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32).bfloat16()
    return (t.view(torch.int16).numpy().astype(np.int64) & 0xffff).astype(np.uint32)


def test_bf16_rne_reference_is_torch_bfloat16():
    rng = np.random.default_rng(3)
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    ties = hi | np.uint32(0x8000)                                   # every tie
    bits = np.concatenate([
        rng.integers(0, 1 << 32, 1 << 24, dtype=np.uint64).astype(np.uint32),
        ties, ties - 1, ties + 1, hi,
        np.array([0x7f7fffff, 0xff7fffff,                          # the largest finite value: rounds up to inf
                  0x7f7f7fff, 0x7f7f8000, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00008001,
                  0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fbfffff, 0x7fffffff, 0x7f80ffff], np.uint32)])
    ref, tor = D.bf16_rne_bits(bits), _torch_bf16_bits(bits)
    nan = D.is_nan_f32_bits(bits)
    assert nan.sum() > 1000 and (~nan).sum() > (1 << 24)
    assert np.array_equal(ref[~nan], tor[~nan])
    assert np.all(D.is_nan_bf16(tor[nan]))                          # quiet and signalling NaN stay NaN; the payload is torch's own
    assert int(D.bf16_rne_bits(np.uint32(0x7f7fffff))) == 0x7f80 and int(D.bf16_rne_bits(np.uint32(0x3f808000))) == 0x3f80
    assert int(D.bf16_rne_bits(np.uint32(0x3f818000))) == 0x3f82


def test_tanh_bf_bound_value():
    """The derived bound of tanh_bf (test_devmath_gpu.py) is a number near 4e-7, reached on the negative side where
    2 / (e + 1) lies in (1, 2)."""
    b = D.tanh_bf_bound()
    print(f"tanh_bf derived absolute-error bound: {b:.4e}")
    assert 3.5e-7 < b < 4.5e-7

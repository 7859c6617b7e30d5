"""The exact-division primitives of the fast kernels, run on the device by the functions the
scheduling kernels call (kss_device_fastmath: csrc/kss_fastmath.cuh, least_bf of kss_simple.cuh,
div_i64 / div_f53 of kss_eval.cuh) with the reciprocals formed as those kernels form them --
v_rcp_f32 for small_div, the device's own f64 division 1.0 / (double)A for the rest -- and compared
for equality with exact integer floor division and the correctly rounded IEEE quotient.

tests/test_fastmath.py checks the same identities on a host copy with a modelled reciprocal; this
file checks the real instructions: that 1.0 / (double)A is correctly rounded on the device
(Markstein's step in div_rn_d needs it), that v_rcp_f32 stays within the 1 ulp the host model
assumes, and every primitive on the operand classes of tests/value_edge_fixtures.py plus every
x in {k d - 1, k d, k d + 1}, k <= 100.  One launch per op; 2^16 .. 2^20 operands each."""
import numpy as np
import pytest

import value_edge_fixtures as vx
from kss import native

pytestmark = pytest.mark.gpu

_CACHE = {}


def _caps():
    """Divisors of the f64 primitives: the fixtures' special, round and searched capacities, small
    values, and a Weyl sequence over [1, 2^46)."""
    if "caps" not in _CACHE:
        xo = vx.x_operands()
        caps = set(vx.SPECIAL_CAPS + vx.ROUND_CAPS + list(range(1, 40)))
        for v in xo.values():
            caps.update(c for c, _ in v[:150])
        caps.update(1 + (i * 0x9E3779B97F4A7C15) % (vx.E46 - 1) for i in range(1, 300))
        caps.update(1 + ((i * 0x9E3779B97F4A7C15) % (vx.E46 - 1) >> (i % 40)) for i in range(1, 120))
        _CACHE["caps"] = np.array(sorted(caps), dtype=np.int64)
        assert 0 < _CACHE["caps"].min() and _CACHE["caps"].max() == vx.E46 - 1
    return _CACHE["caps"]


def _quotient_operands():
    """(x, A): x in {k A - 1, k A, k A + 1} for k = 0 .. 100 at every capacity, plus the searched
    operands (x = (A - R) * 100) of every class -- quotients at most 100, x < 2^53."""
    if "quot" not in _CACHE:
        A = np.repeat(_caps(), 303)
        k = np.tile(np.repeat(np.arange(101, dtype=np.int64), 3), len(_caps()))
        e = np.tile(np.array([-1, 0, 1], dtype=np.int64), 101 * len(_caps()))
        x = k * A + e
        keep = x >= 0
        xs, As = [x[keep]], [A[keep]]
        for v in vx.x_operands().values():
            xs.append(np.array([(c - r) * 100 for c, r in v], dtype=np.int64))
            As.append(np.array([c for c, _ in v], dtype=np.int64))
        x, A = np.concatenate(xs), np.concatenate(As)
        assert x.max() < vx.E53 and (1 << 16) <= len(x) <= (1 << 20)
        _CACHE["quot"] = (x, A)
    return _CACHE["quot"]


def _requested_operands():
    """(requested, capacity) for the score primitives: requested = A - x / 100 around every
    k A / 100 (so that x = (A - requested) * 100 lands on, below and above k A), requested == A,
    requested > A up to 2^52, requested 0, and the searched operands."""
    if "req" not in _CACHE:
        caps = _caps()
        A = np.repeat(caps, 303)
        k = np.tile(np.repeat(np.arange(101, dtype=np.int64), 3), len(caps))
        e = np.tile(np.array([-1, 0, 1], dtype=np.int64), 101 * len(caps))
        r = A - (k * A) // 100 + e   # k = 0: A - 1, A, A + 1; k = 100: -1 (dropped), 0, 1
        keep = r >= 0
        rs, As = [r[keep]], [A[keep]]
        for v in vx.x_operands().values():
            rs.append(np.array([q for _, q in v], dtype=np.int64))
            As.append(np.array([c for c, _ in v], dtype=np.int64))
        over = np.array([2, 3, 1 << 20, (1 << 46) + 1, vx.E52 - 1], dtype=np.int64)
        rs.append(np.minimum(np.repeat(caps, len(over)) + np.tile(over, len(caps)), vx.E52 - 1))
        As.append(np.repeat(caps, len(over)))
        r, A = np.concatenate(rs), np.concatenate(As)
        assert (1 << 16) <= len(r) <= (1 << 20) and (r > A).sum() > 1000 and (r == A).sum() >= len(caps)
        _CACHE["req"] = (r, A)
    return _CACHE["req"]


def _fraction_operands():
    """(a, b) for the f64 quotient: the requested operands (fractions around every hundredth, 1, and
    far above 1), quarters and halves, and numerators up to 2^52 over small and large divisors."""
    if "frac" not in _CACHE:
        r, A = _requested_operands()
        caps = _caps()
        big = np.array([(i * 0x9E3779B97F4A7C15) % vx.E52 for i in range(1, 20001)], dtype=np.int64)
        a = np.concatenate([r, big, np.repeat(caps, 4) * np.tile(np.arange(1, 5, dtype=np.int64), len(caps)) // 4])
        b = np.concatenate([A, caps[np.arange(20000) % len(caps)], np.repeat(caps, 4)])
        _CACHE["frac"] = (a, b)
    return _CACHE["frac"]


def _bits(f):
    return np.asarray(f, dtype=np.float64).view(np.int64)


def _spot_check(a, b, want, f, n=500):
    """The vectorised expectation against plain Python integers on a sample."""
    for i in range(0, len(a), max(len(a) // n, 1)):
        assert int(want[i]) == f(int(a[i]), int(b[i])), (i, int(a[i]), int(b[i]))


def _assert_equal(op, a, b, got, want):
    bad = np.nonzero(got != want)[0]
    print(op, "operands", len(a), "mismatches", len(bad))
    assert len(bad) == 0, (op, len(bad), [(int(a[i]), int(b[i]), int(got[i]), int(want[i])) for i in bad[:8]])


def test_f64_reciprocal_is_correctly_rounded():
    """1.0 / (double)A on the device, bit for bit: the premise of div_rn_d's second residual step."""
    caps = np.concatenate([_caps(), np.array([(i * 0x9E3779B97F4A7C15) % vx.E53 + 1 for i in range(1, 70000)], dtype=np.int64)])
    got = native.device_fastmath("rcp_f64", np.zeros_like(caps), caps)
    _assert_equal("rcp_f64", caps, caps, got, _bits(1.0 / caps.astype(np.float64)))


def test_f32_reciprocal_within_one_ulp():
    """v_rcp_f32 against the correctly rounded float reciprocal: tests/csrc/fastmath_check.c models it
    as that value +- 1 ulp; the largest distance seen is printed."""
    ops = np.array(vx.small_div_operands(), dtype=np.int64)
    d = np.unique(ops[:, 1])
    got = native.device_fastmath("rcp_f32", np.zeros_like(d), d).astype(np.int32)
    want = (np.float32(1.0) / d.astype(np.float32)).view(np.int32)
    dist = np.abs(got.astype(np.int64) - want.astype(np.int64))  # positive floats: bit distance == ulps
    print("v_rcp_f32: divisors", len(d), "max ulp distance", int(dist.max()), "inexact", int((dist > 0).sum()))
    assert dist.max() <= 1, [(int(x), int(g), int(w)) for x, g, w in zip(d[dist > 1][:8], got[dist > 1][:8], want[dist > 1][:8])]


def test_small_div():
    ops = np.array(vx.small_div_operands(), dtype=np.int64)
    x, d = ops[:, 0].copy(), ops[:, 1].copy()
    want = x // d
    _spot_check(x, d, want, lambda p, q: p // q)
    _assert_equal("small_div", x, d, native.device_fastmath("small_div", x, d), want)


@pytest.mark.parametrize("op", ["quot_small_d", "quot_small_i64", "div_f53"])
def test_small_quotients(op):
    x, A = _quotient_operands()
    want = x // A
    _spot_check(x, A, want, lambda p, q: p // q)
    assert want.max() <= 101
    _assert_equal(op, x, A, native.device_fastmath(op, x, A), want)


@pytest.mark.parametrize("op", ["div_rn_d", "div_rn"])
def test_f64_quotient_is_correctly_rounded(op):
    a, b = _fraction_operands()
    want = _bits(a.astype(np.float64) / b.astype(np.float64))  # operands below 2^53 convert exactly
    _spot_check(a, b, want, lambda p, q: int(np.float64(p / q).view(np.int64)))
    _assert_equal(op, a, b, native.device_fastmath(op, a, b), want)


@pytest.mark.parametrize("op", ["least_bf", "alloc_score_d_least", "alloc_score_fast_least", "alloc_score_d_most",
                                "alloc_score_fast_most"])
def test_allocation_scores(op):
    r, A = _requested_operands()
    if op.endswith("most"):
        want = np.minimum(r, A) * 100 // A
        _spot_check(r, A, want, lambda p, q: vx.least_or_most("most", p, q))
    else:
        want = np.where(r > A, 0, (A - np.minimum(r, A)) * 100 // A)
        _spot_check(r, A, want, lambda p, q: vx.least_or_most("least", p, q))
    assert want.min() == 0 and want.max() == 100
    _assert_equal(op, r, A, native.device_fastmath(op, r, A), want)


def test_div_i64_across_2_53():
    """div_i64<false> switches from the f64 division to the integer division at operands of 2^53:
    dividends and divisors on both sides of it, large and small quotients, and the Fit operands
    (capacity - requested) * 100 of capacities between 2^46 and 2^56 stepping across 2^53."""
    E = vx.E53
    edge = [E - 2, E - 1, E, E + 1, E + 2, 2 * E - 1, 2 * E, (1 << 56) - 1, (1 << 62) - 1, (1 << 62) + 12345]
    small = [1, 2, 3, 7, 100, 101, (1 << 31) - 1, (1 << 46) - 1, 1 << 46, (1 << 52) + 1]
    a, b = [], []
    for p in edge + small:
        for q in edge + small:
            a.append(p)
            b.append(q)
    for i in range(1, 40000):  # Weyl operands of every magnitude, each shifted to straddle 2^53
        w = (i * 0x9E3779B97F4A7C15) % (1 << 62)
        v = ((i * 0xBF58476D1CE4E5B9) % (1 << 62)) >> (i % 61)
        a += [w >> (i % 12), E - 1 + (i % 3) - (w >> 40) * (i % 2)]
        b += [max(v, 1), max(v >> 8, 1)]
    for cap in [vx.E46, vx.E46 + 1, (1 << 47) - 1, (1 << 50) + 3, (1 << 53) // 100, (1 << 53) // 100 + 1, (1 << 55) - 1, (1 << 56) - 1]:
        for k in range(0, 101):
            for e in (-1, 0, 1):
                r = cap - (k * cap) // 100 + e
                if 0 <= r <= cap:
                    a.append((cap - r) * 100)
                    b.append(cap)
        for x in (E - 100, E, E + 100):  # (capacity - requested) * 100 on either side of 2^53
            if x // 100 <= cap:
                a.append(x // 100 * 100)
                b.append(cap)
    a, b = np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)
    assert (a >= 0).all() and (b > 0).all() and (1 << 16) <= len(a)
    assert ((a >= E) & (b < E)).sum() > 1000 and ((a < E) & (b >= E)).sum() > 100 and ((a < E) & (b < E)).sum() > 1000
    want = a // b
    assert want.max() > (1 << 53) and (want == 0).sum() > 100
    _spot_check(a, b, want, lambda p, q: p // q, n=3000)
    _assert_equal("div_i64", a, b, native.device_fastmath("div_i64", a, b), want)


def test_probe_refuses_operands_outside_a_primitive():
    with pytest.raises(native.KssError):
        native.device_fastmath("small_div", [1 << 31], [3])
    with pytest.raises(native.KssError):
        native.device_fastmath("quot_small_d", [5], [0])

"""The pre-selection threshold of the range tile kernels (bf_range_mfma.hip), re-derived on the CPU:
for random and adversarial pairs the direct and the expanded form in float32, in several summation
orders, one rounding per step as in an fma chain.  With r = d_dir, the smallest radius that admits the
pair, the kernel's compare must keep it: !(fl(d_e - c |b|^2) > t), cosine !(d_e > r + band)."""
import numpy as np
import pytest

f32, U = np.float32, np.float32(2.0 ** -24)
ORDERS = ("forward", "backward", "strided")


def chain(x, y, order):
    """sum x*y in float32, one rounding per step (exact products in float64), in the given order"""
    p = x.astype(np.float64) * y.astype(np.float64)
    p = p[..., ::-1] if order == "backward" else p
    p = np.concatenate([p[..., s::4] for s in range(4)], -1) if order == "strided" else p
    acc = np.zeros(p.shape[:-1], f32)
    for i in range(p.shape[-1]):
        acc = (acc.astype(np.float64) + p[..., i]).astype(f32)
    return acc


def thresholds(r, qn, D, l2):
    """bf_range_thr_kernel and the host's c (bf_range_mfma.hip) restated: their constants, change together"""
    Df = f32(D)
    if l2:
        c = f32(1.02) * (f32(2) * Df + f32(8)) * U
        t = r / (f32(1) - f32(1.02) * (Df + f32(3)) * U)
        t = (c.astype(np.float64) * qn + t).astype(f32)          # fmaf
        t = t + (f32(2) * Df + f32(8)) * f32(2.3509887e-38)
    else:
        c = f32(0)
        t = r + f32(2.04) * (f32(2) * Df + f32(8)) * U
    return (t + f32(16) * U * t).astype(f32), c


def pairs(kind, D, n, rng):
    q = rng.standard_normal((n, D))
    x = q + rng.standard_normal((n, D)) * 10.0 ** rng.uniform(-4, 1, (n, 1))
    if kind == "decades":        # norms over 12 decades, the two rows of a pair up to 6 apart
        q = q * 10.0 ** rng.uniform(-6, 6, (n, 1))
        x = x * 10.0 ** rng.uniform(-6, 6, (n, 1))
    elif kind == "offset":       # a large common offset that no shift removes
        q, x = q + 1000.0, x + 1000.0
    elif kind == "denormal":     # coordinates whose squares are denormal or flush to zero
        q, x = q * 1e-21, x * 1e-21
    elif kind == "near":         # almost equal rows: the expanded form cancels
        x = q * (1 + 1e-6 * rng.standard_normal((n, D)))
    return q.astype(f32), x.astype(f32)


@pytest.mark.parametrize("D", (4, 100, 960))
@pytest.mark.parametrize("kind", ("plain", "decades", "offset", "denormal", "near"))
def test_l2_threshold_keeps_every_hit(kind, D):
    rng = np.random.default_rng(D + len(kind))
    q, x = pairs(kind, D, 300, rng)
    mu = x.mean(0).astype(f32) if kind in ("plain", "near") else np.zeros(D, f32)
    a, b = (q - mu).astype(f32), (x - mu).astype(f32)
    diff = (q - x).astype(f32)
    for od in ORDERS:
        d_dir = chain(diff, diff, od)
        for oe in ORDERS:
            qn, bn, dot = chain(a, a, oe), chain(b, b, oe), chain(a, b, oe)
            d_e = (f32(-2).astype(np.float64) * dot + (qn + bn).astype(f32)).astype(f32)
            t, c = thresholds(d_dir, qn, D, True)
            lhs = (d_e.astype(np.float64) - c.astype(np.float64) * bn).astype(f32)
            assert not (lhs > t).any(), (od, oe, np.nonzero(lhs > t)[0][:5])


@pytest.mark.parametrize("D", (4, 100, 960))
@pytest.mark.parametrize("kind", ("plain", "decades", "offset", "near"))
def test_cosine_threshold_keeps_every_hit(kind, D):
    rng = np.random.default_rng(50 + D + len(kind))
    q, x = pairs(kind, D, 300, rng)

    def cos_form(qq, bb, dot):
        n2 = (qq * bb).astype(f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.abs(f32(1) - (dot / np.sqrt(n2).astype(f32)).astype(f32)).astype(f32)
        return np.where(n2 > 0, d, f32(1))

    for od in ORDERS:
        d_dir = cos_form(chain(q, q, od), chain(x, x, od), chain(q, x, od))
        for oe in ORDERS:
            d_e = cos_form(chain(q, q, oe), chain(x, x, oe), chain(q, x, oe))
            t, _ = thresholds(d_dir, None, D, False)
            assert not (d_e > t).any(), (od, oe)


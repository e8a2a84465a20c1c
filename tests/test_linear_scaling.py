"""The linear stages (IMDCT, QMF analysis, QMF synthesis with bias 0) at the edges of the float range, in the oracle.

* Exact power-of-two scaling: where no intermediate leaves the normal range, f(x 2^k) == f(x) 2^k bit for bit
  (k = +-20, +-60).
* Subnormal range (analysis and synthesis with scale 1): inputs at 2^-140 (2^-134 for the 1/64-scaled IMDCT, 2^-136
  for synthesis), so that lines, rings and outputs are all subnormal, against a float64 reference: the direct formula
  (IMDCT: test_oracle_fft.imdct_ref; analysis: ISO/IEC 14496-3 4.6.18.4.1, as in test_oracle_props) and, for every
  stage, the stage at unit scale scaled back down in float64.  Bound: REL * max|ref| + ULPS subnormal ulps (2^-149);
  a flush-to-zero gives 0 where the reference is over a thousand ulps from zero.

test_edges_gpu.py runs the same checks on the HIP stages (STAGES takes either implementation)."""
import numpy as np
import pytest

from test_oracle_fft import imdct_ref

IMDCT = {0: (2048, 1.0), 1: (256, 1.0), 2: (128, 1.0 / 64), 3: (128, -2.0)}     # which: (n, scale)
SCALES = (20, -20, 60, -60)
SUB = -140
SUB_AT = {"imdct2": -134, "synthesis": -136, "synthesis_ds": -136}
ULP = 2.0 ** -149
REL = 2e-5            # the normal-range accuracy of the float stages against float64 (test_oracle_fft, _props)
ULPS = 64             # rounding of the subnormal intermediates, in ulps


class OracleStages:
    """the stages on [n][...] arrays; each returns a tuple of outputs (state last)"""

    def __init__(self, oracle):
        self.o = oracle

    def imdct(self, which, x):
        return (self.o.imdct_half(which, x),)

    def analysis(self, x, xh):
        r = [self.o.qmf_analysis(x[i], xh[i], scale=1.0) for i in range(x.shape[0])]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def synthesis(self, X, v):
        r = [self.o.qmf_synthesis(X[i], v[i], scale=1.0, bias=0.0) for i in range(X.shape[0])]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def synthesis_ds(self, X, v):
        r = [self.o.qmf_synthesis_ds(X[i], v[i], scale=1.0, bias=0.0) for i in range(X.shape[0])]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])


def inputs(name, n, seed):
    """unit-level inputs of a stage (its lines / samples and its ring)"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    if name.startswith("imdct"):
        return (f(n, IMDCT[int(name[-1])][0] // 2),)
    if name == "analysis":
        return f(n, 1024), f(n, 288)
    if name == "synthesis":
        return f(n, 2, 32, 64), f(n, 1152)
    return f(n, 2, 32, 64), f(n, 576)


def run(impl, name, args):
    if name.startswith("imdct"):
        return impl.imdct(int(name[-1]), *args)
    return getattr(impl, name)(*args)


STAGES = ["imdct0", "imdct1", "imdct2", "imdct3", "analysis", "synthesis", "synthesis_ds"]


def _p2(a, k):
    return (np.asarray(a, np.float64) * 2.0 ** k).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_power_of_two_scaling(impl, name, n=3, seed=1):
    args = inputs(name, n, seed)
    base = run(impl, name, args)
    for k in SCALES:
        got = run(impl, name, tuple(_p2(a, k) for a in args))
        for g, b in zip(got, base):
            assert np.all(np.isfinite(b)) and np.abs(b[b != 0]).min() * 2.0 ** k >= 2.0 ** -126
            assert np.array_equal(_bits(g), _bits(_p2(b, k))), (name, k)


def direct_reference(name, args):
    """float64 direct formula of the first output, where there is one (None otherwise)"""
    if name.startswith("imdct"):
        which = int(name[-1])
        n, scale = IMDCT[which]
        return np.stack([imdct_ref(x, n)[n // 4: 3 * n // 4] * scale for x in args[0]])
    if name == "analysis":
        import oracle_lib
        c = oracle_lib.get_table("qmf_ds").astype(np.float64)
        m = np.arange(64)
        k = np.arange(32)[:, None]
        M = 2 * np.exp(1j * np.pi / 64 * (k + 0.5) * (2 * m[None, :] - 0.5))
        out = []
        for x, xh in zip(*args):
            buf = np.concatenate([xh.astype(np.float64), x.astype(np.float64)])
            W = np.stack([M @ (c * buf[32 * i: 32 * i + 320][::-1]).reshape(5, 64).sum(axis=0) for i in range(32)])
            out.append(np.stack([W.real, W.imag], axis=-1))
        return np.stack(out)
    return None


def check_subnormal_range(impl, ref_impl, name, n=3, seed=2):
    """inputs at 2^-140 against float64: the direct formula and the stage at unit scale, scaled down"""
    args = inputs(name, n, seed)
    e = SUB_AT.get(name, SUB)
    sub = tuple(_p2(a, e) for a in args)
    got = run(impl, name, sub)
    refs = [np.asarray(r, np.float64) * 2.0 ** e for r in run(ref_impl, name, args)]
    direct = direct_reference(name, sub)
    if direct is not None:
        refs[0] = direct
    for g, r in zip(got, refs):
        g = np.asarray(g, np.float64)
        bound = REL * np.abs(r).max() + ULPS * ULP
        err = np.abs(g - r).max()
        assert err <= bound, (name, err / ULP, bound / ULP)
        assert np.abs(r).max() > 20 * bound            # the reference is far from zero: a flush cannot pass
        assert np.any((g != 0) & (np.abs(g) < 2.0 ** -126))


@pytest.mark.parametrize("name", STAGES)
def test_oracle_power_of_two_scaling(oracle, name):
    check_power_of_two_scaling(OracleStages(oracle), name)


@pytest.mark.parametrize("name", STAGES)
def test_oracle_subnormal_range(oracle, name):
    s = OracleStages(oracle)
    check_subnormal_range(s, s, name)

"""The spectral tools on the GPU over the structural profiles of tests/edge_tools.py -- every band table, TNS order,
grouping and predictor reset group (tests/test_tools_reach.py counts what the records hold) -- through every form of
the call: chained heaac_spectral_tools_batch calls, one heaac_spectral_tools_streams call over all frames (the chain
kernel and k_tns), heaac_spectral_tools_batch_ex with an empty coupling slot (TNS inside the frame's wave:
tools_tns_filter) and, for two profiles, heaac_spectral_tools_streams_ex with a mask that holds nothing (the masked
instantiations).  Against the oracle chained frame by frame: every coefficient and predictor word bit-identical, the
generator word equal, a NaN matched by any NaN."""
import numpy as np
import pytest

import edge_tools as E

pytestmark = pytest.mark.gpu

CASES = list(E.CASES)                # (profile, the state the run carries)
HOLD_CASES = [c for c in CASES if c[0] in ("tns_orders", "prediction")]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_words(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ok = (_bits(got) == _bits(ref)) | (np.isnan(got) & np.isnan(ref))
    assert ok.all(), "%s: %d words differ, first at %s" % (what, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


def _assert_same(got, ref, what):
    """(coefficients, generator, predictors) against the oracle's; None: the run does not carry that state"""
    _assert_words(got[0], ref[0], what + " coefficients")
    for k, name in ((1, " generator"), (2, " predictors")):
        assert (got[k] is None) == (ref[k] is None), what + name
    if ref[1] is not None:
        assert np.array_equal(got[1], ref[1]), what + " generator"
    if ref[2] is not None:
        _assert_words(got[2], ref[2], what + " predictors")


def _dev_t(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _host(t):
    return None if t is None else t.cpu().numpy()


def _case(pkg, oracle, profile, channels, state):
    coeffs, tools = E.frames(pkg, profile, channels)
    rs, pred = E.start_state(pkg, tools.shape[0], channels, state)
    return coeffs, tools, rs, pred, E.oracle_chain(pkg, oracle, profile, channels, state)


def _chained(pkg, coeffs, tools, rs, pred, ref, call, what):
    """`call(d_coeffs, d_tools, d_rs, d_pred)` frame position by frame position, the state in place, compared with
    the oracle after every frame"""
    d_rs, d_pred = _dev_t(rs), _dev_t(pred)
    for t in range(tools.shape[1]):
        d = _dev_t(coeffs[:, t])
        call(d, pkg.to_device(np.array(tools[:, t])), d_rs, d_pred)
        _assert_same((_host(d), _host(d_rs), _host(d_pred)), ref[t], "%s frame %d" % (what, t))


def _streams(pkg, dev, channels, coeffs, tools, rs, pred, ref, hold=None):
    S, T = tools.shape
    d = _dev_t(coeffs.reshape((S * T,) + coeffs.shape[2:]))
    d_rs, d_pred = _dev_t(rs), _dev_t(pred)
    dev.spectral_tools_streams(channels, d, pkg.to_device(np.array(tools.reshape(-1))), T, rng=d_rs, pred=d_pred,
                               hold=hold)
    got = _host(d).reshape(coeffs.shape)
    for t in range(T):
        _assert_words(got[:, t], ref[t][0], "frame %d coefficients" % t)
    _assert_same((got[:, T - 1], _host(d_rs), _host(d_pred)), ref[T - 1], "end of the chain")


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile,state", CASES)
def test_batch_calls_chained(pkg, oracle, dev, profile, state, channels):
    coeffs, tools, rs, pred, ref = _case(pkg, oracle, profile, channels, state)
    _chained(pkg, coeffs, tools, rs, pred, ref,
             lambda d, t, r, p: dev.spectral_tools(channels, d, t, rng=r, pred=p), "batch")


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile,state", CASES)
def test_one_streams_call(pkg, oracle, dev, profile, state, channels):
    coeffs, tools, rs, pred, ref = _case(pkg, oracle, profile, channels, state)
    _streams(pkg, dev, channels, coeffs, tools, rs, pred, ref)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile,state", CASES)
def test_tns_inside_the_wave_with_nothing_coupled(pkg, oracle, dev, profile, state, channels):
    """one coupling slot with present = 0 and a zero spectrum: TNS moves from k_tns into the frame's wave and the
    result is the plain call's"""
    import torch
    coeffs, tools, rs, pred, ref = _case(pkg, oracle, profile, channels, state)
    S = tools.shape[0]
    cce = pkg.to_device(np.zeros((S, 1), pkg.CCE_FRAME_DT))
    cce_coeffs = torch.zeros((S, 1, 1024), dtype=torch.float32, device="cuda")
    _chained(pkg, coeffs, tools, rs, pred, ref,
             lambda d, t, r, p: dev.spectral_tools_ex(channels, pkg.TOOLS_ALL, d, t, rng=r, pred=p, cce=cce,
                                                      cce_coeffs=cce_coeffs), "in-wave TNS")
    assert not cce_coeffs.any()


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile,state", HOLD_CASES)
def test_streams_call_with_a_mask_that_holds_nothing(pkg, oracle, dev, profile, state, channels):
    import torch
    coeffs, tools, rs, pred, ref = _case(pkg, oracle, profile, channels, state)
    _streams(pkg, dev, channels, coeffs, tools, rs, pred, ref,
             hold=torch.zeros(tools.size, dtype=torch.uint8, device="cuda"))

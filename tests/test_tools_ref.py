"""oracle/or_tools.c against an independent restatement (tests/tools_ref.py: numpy float32, written from the
reference's text and vectorised across lines, bands and filters where the oracle loops as the reference does): every
coefficient word, generator word and predictor word identical on all four profiles of tests/edge_tools.py, mono and
stereo, state chained.  Each tool is a sequence of singly-rounded float32 operations, so there is no tolerance; a NaN
is matched by any NaN.  CPU only."""
import numpy as np
import pytest

import edge_tools as E
import tools_ref as R


def _same_words(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ok = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert ok.all(), "%s: %d words differ, first at %s" % (what, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", E.PROFILES)
def test_restatement_equals_oracle(pkg, oracle, profile, channels):
    coeffs, tools = E.frames(pkg, profile, channels)
    chain = E.oracle_chain(pkg, oracle, profile, channels, "pns_main")
    rs, pred = E.start_state(pkg, tools.shape[0], channels, "pns_main")
    for t in range(tools.shape[1]):
        out, rs, pred = R.spectral_tools_batch(channels, coeffs[:, t], tools[:, t], rs, pred)
        _same_words(out, chain[t][0], "frame %d coefficients" % t)
        assert np.array_equal(rs, chain[t][1]), "frame %d generator" % t
        _same_words(pred, chain[t][2], "frame %d predictors" % t)


@pytest.mark.parametrize("channels", [1, 2])
def test_restatement_equals_oracle_without_state(pkg, oracle, channels):
    """no generator, no predictors: noise bands are taken as given (tables, the profile the GPU runs both ways)"""
    coeffs, tools = E.frames(pkg, "tables", channels)
    chain = E.oracle_chain(pkg, oracle, "tables", channels, "none")
    for t in range(tools.shape[1]):
        _same_words(R.spectral_tools_batch(channels, coeffs[:, t], tools[:, t]), chain[t][0], "frame %d" % t)


def test_generator_table_is_the_serial_generator():
    """the composed steps of tools_ref against lcg_random (aacdec.c:502-505) run one step at a time"""
    x = 0x1f2e3d4c
    for j in range(1, 1025):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        assert int(R._A[j]) * 0x1f2e3d4c + int(R._C[j]) & 0xffffffff == x, j

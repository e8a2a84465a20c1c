"""heaac_he_decode_streams without a GPU: the entry point is declared and exported, it refuses a NULL device, and the
Python wrapper checks every tensor's length before anything reaches the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1


def test_streams_entry_point_declared_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_dsp.h")).read()
    assert re.search(r"\bint\s+heaac_he_decode_streams\s*\(", txt)
    assert "heaac_he_decode_streams" in pkg.EXPORTED
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    assert "heaac_he_decode_streams" in {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_streams_null_device_is_refused(pkg):
    L = pkg.lib()
    f = L.heaac_he_decode_streams
    dummy = C.c_void_p(16)
    for cfg in (pkg.CFG_HEV1, pkg.CFG_HEV1_MONO, pkg.CFG_HEV2):
        for S, T in ((1, 1), (4, 8), (0, 1)):
            rc = f(None, cfg, 0, dummy, dummy, dummy, dummy, 1, dummy, dummy, dummy, dummy, pkg.PCM_F32, S, T, None)
            assert rc == HEAAC_ERR_ARG, (cfg, S, T, rc)
    assert L.heaac_strerror(HEAAC_ERR_ARG)


class _NoDevice:
    """Stands in for the library: the wrapper must not get as far as calling it."""
    def __getattr__(self, name):
        raise AssertionError("device call %s reached" % name)


def _tensors(pkg, cfg, S, T):
    import torch
    n = S * T
    nc = pkg.CORE_CH[cfg]
    return dict(
        coeffs=torch.zeros(n * nc * 1024, dtype=torch.float32),
        ics=torch.zeros(n * nc * pkg.ICS_DT.itemsize, dtype=torch.uint8),
        sbr=torch.zeros(n * pkg.SBR_FRAME_DT.itemsize, dtype=torch.uint8),
        hdr=torch.zeros(pkg.SBR_HDR_DT.itemsize, dtype=torch.uint8),
        ps=torch.zeros(n * pkg.PS_FRAME_DT.itemsize, dtype=torch.uint8) if cfg == pkg.CFG_HEV2 else None,
        state_in=torch.zeros(S * pkg.STATE_WORDS[cfg], dtype=torch.float32))


@pytest.mark.parametrize("which", ["coeffs", "ics", "sbr", "ps", "state_out", "pcm"])
def test_streams_wrapper_rejects_wrong_lengths(pkg, monkeypatch, which):
    import torch
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    cfg, S, T = pkg.CFG_HEV2, 3, 4
    a = _tensors(pkg, cfg, S, T)
    kw = {}
    if which in ("coeffs", "ics", "sbr", "ps"):
        a[which] = a[which][:-1]                     # one element short
    elif which == "state_out":
        kw["state_out"] = torch.zeros(S * pkg.STATE_WORDS[cfg] + 1, dtype=torch.float32)
    else:
        kw["pcm"] = torch.zeros(S * (T - 1) * 2 * 2048, dtype=torch.float32)   # sized for T - 1 frames
    with pytest.raises(AssertionError) as e:
        dev.he_decode_streams(cfg, a["coeffs"], a["ics"], a["sbr"], a["hdr"], a["ps"], a["state_in"], T, **kw)
    assert which in str(e.value)


def test_streams_wrapper_sizes_by_stream_count(pkg, monkeypatch):
    """state_in has one record per STREAM: per-frame tensors sized for S frames (the batch call's layout with one
    frame per stream) are refused when T > 1."""
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    cfg, S, T = pkg.CFG_HEV1, 5, 2
    a = _tensors(pkg, cfg, S, 1)
    with pytest.raises(AssertionError) as e:
        dev.he_decode_streams(cfg, a["coeffs"], a["ics"], a["sbr"], a["hdr"], None, a["state_in"], T)
    assert "coeffs" in str(e.value)
    np.testing.assert_equal(pkg.STATE_WORDS[cfg], a["state_in"].numel() // S)

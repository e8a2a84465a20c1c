"""heaac_lc_decode_streams without a GPU: the entry point is declared and exported, it refuses a NULL device, and the
Python wrapper checks every tensor's length before anything reaches the device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1


def test_lc_streams_entry_point_declared_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_dsp.h")).read()
    assert re.search(r"\bint\s+heaac_lc_decode_streams\s*\(", txt)
    assert "heaac_lc_decode_streams" in pkg.EXPORTED
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    assert "heaac_lc_decode_streams" in {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_lc_streams_null_device_is_refused(pkg):
    L = pkg.lib()
    f = L.heaac_lc_decode_streams
    dummy = C.c_void_p(16)
    for channels in (1, 2):
        for S, T in ((1, 1), (4, 8), (0, 1)):
            rc = f(None, channels, dummy, dummy, dummy, dummy, dummy, pkg.PCM_F32, S, T, None)
            assert rc == HEAAC_ERR_ARG, (channels, S, T, rc)


class _NoDevice:
    """Stands in for the library: the wrapper must not get as far as calling it."""
    def __getattr__(self, name):
        raise AssertionError("device call %s reached" % name)


def _tensors(pkg, channels, S, T):
    import torch
    n = S * T
    return dict(coeffs=torch.zeros(n * channels * 1024, dtype=torch.float32),
                ics=torch.zeros(n * channels * pkg.ICS_DT.itemsize, dtype=torch.uint8),
                state_in=torch.zeros(S * channels * 512, dtype=torch.float32))


def _no_device(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    return dev


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("short", ["element", "frame"])
@pytest.mark.parametrize("which", ["coeffs", "ics", "state_in", "state_out", "pcm"])
def test_lc_streams_wrapper_rejects_wrong_lengths(pkg, monkeypatch, which, short, channels):
    """every tensor one element short, or sized for T - 1 frames per stream (the state: for S - 1 streams)"""
    import torch
    dev = _no_device(pkg, monkeypatch)
    S, T = 3, 4
    a = _tensors(pkg, channels, S, T)
    kw = {}
    if which in ("coeffs", "ics"):
        a[which] = a[which][:-1] if short == "element" else _tensors(pkg, channels, S, T - 1)[which]
    elif which == "state_in":
        # one element short no longer holds S whole records; S - 1 records leave the frames T * S / (S - 1) each
        a[which] = a[which][:-1] if short == "element" else _tensors(pkg, channels, S - 1, T)[which]
    elif which == "state_out":
        k = S * channels * 512
        kw["state_out"] = torch.zeros(k - 1 if short == "element" else k - channels * 512, dtype=torch.float32)
    else:
        k = S * T * channels * 1024
        kw["pcm"] = torch.zeros(k - 1 if short == "element" else S * (T - 1) * channels * 1024, dtype=torch.float32)
    with pytest.raises(AssertionError) as e:
        dev.lc_decode_streams(channels, a["coeffs"], a["ics"], a["state_in"], T, **kw)
    want = "coeffs" if which == "state_in" and short == "frame" else which
    assert want in str(e.value)


@pytest.mark.parametrize("fmt", ["PCM_S16", "PCM_S16_SSE2"])
def test_lc_streams_wrapper_checks_int16_pcm(pkg, monkeypatch, fmt):
    import torch
    dev = _no_device(pkg, monkeypatch)
    S, T = 5, 2
    a = _tensors(pkg, 2, S, T)
    for bad in (torch.zeros(S * (T - 1) * 1024 * 2, dtype=torch.int16),          # T - 1 frames
                torch.zeros(S * T * 1024 * 2, dtype=torch.float32)):            # the F32 buffer
        with pytest.raises(AssertionError) as e:
            dev.lc_decode_streams(2, a["coeffs"], a["ics"], a["state_in"], T, pcm=bad, pcm_format=getattr(pkg, fmt))
        assert "pcm" in str(e.value)


def test_lc_streams_wrapper_sizes_by_stream_count(pkg, monkeypatch):
    """state_in has one record per STREAM: per-frame tensors sized for S frames (the batch call's layout with one
    frame per stream) are refused when T > 1."""
    dev = _no_device(pkg, monkeypatch)
    S, T = 5, 2
    a = _tensors(pkg, 2, S, 1)
    with pytest.raises(AssertionError) as e:
        dev.lc_decode_streams(2, a["coeffs"], a["ics"], a["state_in"], T)
    assert "coeffs" in str(e.value)

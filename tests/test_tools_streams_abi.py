"""heaac_spectral_tools_streams without a GPU: the entry point is declared and exported, it refuses a NULL device, and
the Python wrapper checks every tensor's length and dtype before anything reaches the device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1


def test_tools_streams_entry_point_declared_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_dsp.h")).read()
    assert re.search(r"\bint\s+heaac_spectral_tools_streams\s*\(", txt)
    assert "heaac_spectral_tools_streams" in pkg.EXPORTED
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    assert "heaac_spectral_tools_streams" in {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_tools_streams_null_device_is_refused(pkg):
    L = pkg.lib()
    f = L.heaac_spectral_tools_streams
    dummy = C.c_void_p(16)
    for channels in (1, 2):
        for S, T in ((1, 1), (4, 8), (0, 1)):
            for state in ((dummy,) * 4, (None,) * 4):
                rc = f(None, channels, dummy, dummy, *state, S, T, None)
                assert rc == HEAAC_ERR_ARG, (channels, S, T, rc)


class _DeviceReached(Exception):
    """Not an AssertionError: a call that got past the wrapper's checks must not pass for one they raised."""


class _NoDevice:
    """Stands in for the library: the wrapper must not get as far as calling it."""
    def __getattr__(self, name):
        raise _DeviceReached(name)


def _tensors(pkg, channels, S, T):
    import torch
    n = S * T
    return dict(coeffs=torch.zeros(n * channels * 1024, dtype=torch.float32),
                tools=torch.zeros(n * pkg.TOOLS_FRAME_DT.itemsize, dtype=torch.uint8),
                rng=torch.zeros(S, dtype=torch.int32),
                pred=torch.zeros(S * channels * pkg.MAX_PREDICTORS * 6, dtype=torch.float32))


def _no_device(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    return dev


def _call(dev, channels, a, T, **kw):
    return dev.spectral_tools_streams(channels, a["coeffs"], a["tools"], T, rng=a["rng"], pred=a["pred"], **kw)


@pytest.mark.parametrize("outputs", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_wrapper_passes_right_tensors_on(pkg, monkeypatch, channels, outputs):
    """the control: tensors of the right lengths and dtypes get past every check, as far as the library"""
    dev = _no_device(pkg, monkeypatch)
    S, T = 3, 4
    a = _tensors(pkg, channels, S, T)
    kw = dict(rng_out=a["rng"].clone(), pred_out=a["pred"].clone()) if outputs else {}
    with pytest.raises(_DeviceReached) as e:
        _call(dev, channels, a, T, **kw)
    assert str(e.value) == "heaac_spectral_tools_streams"
    with pytest.raises(_DeviceReached):
        dev.spectral_tools_streams(channels, a["coeffs"], a["tools"], T)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("short", ["element", "record"])
@pytest.mark.parametrize("which", ["tools", "rng", "pred", "rng_out", "pred_out"])
def test_tools_streams_wrapper_rejects_wrong_lengths(pkg, monkeypatch, which, short, channels):
    """every tensor one element short, or sized for one frame per stream less (the state: one stream less)"""
    dev = _no_device(pkg, monkeypatch)
    S, T = 3, 4
    a = _tensors(pkg, channels, S, T)
    kw = {}
    if which == "tools":
        a[which] = a[which][:-1] if short == "element" else _tensors(pkg, channels, S, T - 1)[which]
    elif which in ("rng", "pred"):
        a[which] = a[which][:-1] if short == "element" else _tensors(pkg, channels, S - 1, T)[which]
    else:
        src = _tensors(pkg, channels, S, T)[which[:-4]]
        kw[which] = src[:-1] if short == "element" else _tensors(pkg, channels, S - 1, T)[which[:-4]]
    with pytest.raises(AssertionError) as e:
        _call(dev, channels, a, T, **kw)
    assert which in str(e.value)


@pytest.mark.parametrize("which", ["coeffs", "tools", "rng", "pred", "rng_out", "pred_out"])
def test_tools_streams_wrapper_rejects_wrong_dtypes(pkg, monkeypatch, which):
    import torch
    dev = _no_device(pkg, monkeypatch)
    S, T, channels = 3, 2, 2
    a = _tensors(pkg, channels, S, T)
    kw = {}
    # same byte count or same element count in the wrong type
    wrong = {"coeffs": torch.int32, "tools": torch.int8, "rng": torch.float32, "pred": torch.int32,
             "rng_out": torch.float32, "pred_out": torch.int32}[which]
    if which.endswith("_out"):
        kw[which] = a[which[:-4]].to(wrong)
    else:
        a[which] = a[which].to(wrong)
    with pytest.raises(AssertionError) as e:
        _call(dev, channels, a, T, **kw)
    assert which in str(e.value)


def test_tools_streams_wrapper_frames_must_be_a_multiple_of_T(pkg, monkeypatch):
    dev = _no_device(pkg, monkeypatch)
    a = _tensors(pkg, 2, 1, 7)                    # 7 frames
    for T in (2, 3, 4, 5, 6, 8):
        with pytest.raises(AssertionError) as e:
            dev.spectral_tools_streams(2, a["coeffs"], a["tools"], T)
        assert "frames_per_stream" in str(e.value) or "coeffs" in str(e.value)
    # a partial frame
    with pytest.raises(AssertionError) as e:
        dev.spectral_tools_streams(2, a["coeffs"][:-1], a["tools"], 7)
    assert "coeffs" in str(e.value)


@pytest.mark.parametrize("T", [0, -1])
def test_tools_streams_wrapper_rejects_T_below_one(pkg, monkeypatch, T):
    dev = _no_device(pkg, monkeypatch)
    a = _tensors(pkg, 2, 2, 2)
    with pytest.raises(AssertionError) as e:
        _call(dev, 2, a, T)
    assert "frames_per_stream" in str(e.value)


def test_tools_streams_wrapper_sizes_state_by_stream_count(pkg, monkeypatch):
    """rng / pred hold one record per STREAM: state sized for S * T frames (the batch call's per-frame layout) is
    refused when T > 1, and an output without its input is refused too."""
    dev = _no_device(pkg, monkeypatch)
    S, T, channels = 5, 2, 2
    a = _tensors(pkg, channels, S, T)
    per_frame = _tensors(pkg, channels, S * T, 1)
    for which in ("rng", "pred"):
        b = dict(a)
        b[which] = per_frame[which]
        with pytest.raises(AssertionError) as e:
            _call(dev, channels, b, T)
        assert which in str(e.value)
    for which in ("rng_out", "pred_out"):
        with pytest.raises(AssertionError) as e:
            dev.spectral_tools_streams(channels, a["coeffs"], a["tools"], T, **{which: a[which[:-4]]})
        assert which in str(e.value)

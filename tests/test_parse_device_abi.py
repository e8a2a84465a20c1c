"""heaac_aac_parse_device without a GPU: the call and the host form of its walk are declared and exported, a NULL
device and NULL arrays are refused, and the Python wrapper checks every tensor's length before anything reaches the
library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1


def _cfg(pkg):
    c = pkg.AacConfig()
    c.object_type, c.sampling_index, c.sample_rate, c.chan_config = 2, 3, 48000, 2
    return c


def test_parse_device_entry_points_declared_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_parse.h")).read()
    assert re.search(r"\bint\s+heaac_aac_parse_device\s*\(", txt)
    assert re.search(r"#define\s+HEAAC_PARSE_DEFERRED\s+1\b", txt)
    dbg = open(os.path.join(ROOT, "include", "heaac_debug.h")).read()
    assert re.search(r"\bint\s+heaac_debug_aac_parse_core\s*\(", dbg)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("heaac_aac_parse_device", "heaac_debug_aac_parse_core"):
        assert name in pkg.EXPORTED and name in syms, name
    assert (pkg.PARSE_OK, pkg.PARSE_DEFERRED) == (0, 1)


def test_parse_device_null_device_and_null_arrays_are_refused(pkg):
    f = pkg.lib().heaac_aac_parse_device
    cfg = _cfg(pkg)
    dummy = C.c_void_p(64)
    for n in (0, 1, 4096):
        for cc in (1, 2):
            assert f(None, C.byref(cfg), dummy, dummy, dummy, n, cc, dummy, dummy, dummy, dummy, dummy, None) == HEAAC_ERR_ARG
    # the host form of the same call takes the same arrays: each of them NULL in turn
    g = pkg.lib().heaac_debug_aac_parse_core
    st = np.zeros(1, pkg.AAC_STREAM_DT)
    au = np.zeros(16, np.uint8)
    off = np.array([0, 3], np.uint32)
    co, ic = np.zeros((1, 2, 1024), np.float32), np.zeros((1, 2), pkg.ICS_DT)
    to, inf, status = np.zeros(1, pkg.TOOLS_FRAME_DT), np.zeros(1, pkg.AAC_INFO_DT), np.zeros(1, np.int32)
    args = [C.addressof(cfg), st.ctypes.data, au.ctypes.data, off.ctypes.data, 1, 2, co.ctypes.data, ic.ctypes.data,
            to.ctypes.data, inf.ctypes.data, status.ctypes.data, None]
    assert g(*args) == 0
    for k in (0, 1, 2, 3, 6, 7, 8, 9, 10):
        bad = list(args)
        bad[k] = None
        assert g(*bad) == HEAAC_ERR_ARG, k
    bad = list(args)
    bad[4] = 0
    bad[1] = None
    assert g(*bad) == 0                                   # n = 0: nothing is looked at


class _NoDevice:
    """Stands in for the library: the wrapper must not get as far as calling it."""
    def __getattr__(self, name):
        raise AssertionError("device call %s reached" % name)


def _no_device(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    return dev


def _tensors(pkg, n, cc):
    import torch
    return dict(streams=torch.zeros(n * pkg.AAC_STREAM_DT.itemsize, dtype=torch.uint8),
                coeffs=torch.zeros(n * cc * 1024, dtype=torch.float32),
                ics=torch.zeros(n * cc * pkg.ICS_DT.itemsize, dtype=torch.uint8),
                tools=torch.zeros(n * pkg.TOOLS_FRAME_DT.itemsize, dtype=torch.uint8),
                info=torch.zeros(n * pkg.AAC_INFO_DT.itemsize, dtype=torch.uint8),
                status=torch.zeros(n, dtype=torch.int32))


@pytest.mark.parametrize("cc", [1, 2])
@pytest.mark.parametrize("short", ["element", "unit"])
@pytest.mark.parametrize("which", ["streams", "coeffs", "ics", "tools", "info", "status"])
def test_parse_device_wrapper_rejects_wrong_lengths(pkg, monkeypatch, which, short, cc):
    """every tensor one element short, or sized for n - 1 units"""
    import torch
    dev = _no_device(pkg, monkeypatch)
    n = 5
    a = _tensors(pkg, n, cc)
    a[which] = a[which][:-1] if short == "element" else _tensors(pkg, n - 1, cc)[which]
    au = torch.zeros(100, dtype=torch.uint8)
    off = np.arange(n + 1) * 20
    with pytest.raises(AssertionError) as e:
        dev.aac_parse(_cfg(pkg), a.pop("streams"), au, off, coeff_channels=cc, **a)
    assert which in str(e.value)


def test_parse_device_wrapper_checks_the_offsets(pkg, monkeypatch):
    import torch
    dev = _no_device(pkg, monkeypatch)
    n = 4
    a = _tensors(pkg, n, 2)
    au = torch.zeros(100, dtype=torch.uint8)
    for off in ([0, 20, 40, 60, 101],          # past the end of the bytes
                [0, 40, 20, 60, 80],           # running backwards
                [-1, 20, 40, 60, 80]):
        with pytest.raises(AssertionError) as e:
            dev.aac_parse(_cfg(pkg), a["streams"], au, np.array(off), coeff_channels=2)
        assert "au_offset" in str(e.value)
    with pytest.raises(AssertionError) as e:
        dev.aac_parse(_cfg(pkg), a["streams"], au, np.array([0, 20, 40, 60, 80]), coeff_channels=3)
    assert "coeff_channels" in str(e.value)
    with pytest.raises(AssertionError) as e:
        dev.aac_parse(_cfg(pkg), a["streams"], au.to(torch.int8), np.array([0, 20, 40, 60, 80]))
    assert "au_bytes" in str(e.value)

"""The hold-mask entry points (heaac_*_streams_ex) and the pipeline's streams form (heaac_pipeline_create_streams)
without a GPU: declared, listed and exported; a NULL device is refused; the Python wrappers check the mask's length and
type before anything reaches the device; the create call names its argument errors before it looks for a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1
HEAAC_ERR_NODEVICE = -4

NEW = {"heaac_lc_decode_streams_ex": "heaac_dsp.h", "heaac_he_decode_streams_ex": "heaac_dsp.h",
       "heaac_spectral_tools_streams_ex": "heaac_dsp.h", "heaac_pipeline_create_streams": "heaac_pipeline.h",
       "heaac_pipeline_frames_per_tick": "heaac_pipeline.h"}


@pytest.mark.parametrize("name", sorted(NEW))
def test_new_symbols_declared_listed_and_exported(pkg, name):
    txt = open(os.path.join(ROOT, "include", NEW[name])).read()
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, txt)
    assert name in pkg.EXPORTED
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    assert name in {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_error_codes_are_the_headers(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_dsp.h")).read()
    for name, val in (("HEAAC_ERR_ARG", HEAAC_ERR_ARG), ("HEAAC_ERR_NODEVICE", HEAAC_ERR_NODEVICE)):
        m = re.search(r"\b%s\s*=?\s*\(?(-?\d+)" % name, txt)
        assert m and int(m.group(1)) == val, name


def test_null_device_is_refused(pkg):
    L = pkg.lib()
    dummy = C.c_void_p(16)
    lc = L.heaac_lc_decode_streams_ex
    he = L.heaac_he_decode_streams_ex
    tl = L.heaac_spectral_tools_streams_ex
    for hold in (None, dummy):
        for S, T in ((1, 1), (4, 8), (0, 1)):
            for channels in (1, 2):
                assert lc(None, channels, dummy, dummy, dummy, dummy, dummy, pkg.PCM_F32, S, T, hold, None) == HEAAC_ERR_ARG
                assert tl(None, channels, dummy, dummy, dummy, dummy, None, None, S, T, hold, None) == HEAAC_ERR_ARG
            for cfg in (pkg.CFG_HEV2, pkg.CFG_HEV1, pkg.CFG_HEV1_MONO):
                assert he(None, cfg, 0, dummy, dummy, dummy, dummy, 1, dummy, dummy, dummy, dummy, pkg.PCM_F32, S, T,
                          hold, None) == HEAAC_ERR_ARG


class _NoDevice:
    """Stands in for the library: the wrapper must not get as far as calling it."""
    def __getattr__(self, name):
        raise AssertionError("device call %s reached" % name)


def _no_device(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    return dev


def _bad_holds(S, T):
    import torch
    return {"element": torch.zeros(S * T - 1, dtype=torch.uint8), "frame": torch.zeros(S * (T - 1), dtype=torch.uint8),
            "dtype": torch.zeros(S * T, dtype=torch.int32), "bool": torch.zeros(S * T, dtype=torch.bool)}


@pytest.mark.parametrize("bad", ["element", "frame", "dtype", "bool"])
@pytest.mark.parametrize("channels", [1, 2])
def test_lc_wrapper_rejects_a_wrong_hold(pkg, monkeypatch, channels, bad):
    import torch
    dev = _no_device(pkg, monkeypatch)
    S, T = 3, 4
    n = S * T
    with pytest.raises(AssertionError) as e:
        dev.lc_decode_streams(channels, torch.zeros(n * channels * 1024), torch.zeros(n * channels * pkg.ICS_DT.itemsize,
                                                                                      dtype=torch.uint8),
                              torch.zeros(S * channels * 512), T, hold=_bad_holds(S, T)[bad])
    assert "hold" in str(e.value)


@pytest.mark.parametrize("bad", ["element", "frame", "dtype", "bool"])
@pytest.mark.parametrize("cfgname", ["CFG_HEV2", "CFG_HEV1", "CFG_HEV1_MONO"])
def test_he_wrapper_rejects_a_wrong_hold(pkg, monkeypatch, cfgname, bad):
    import torch
    dev = _no_device(pkg, monkeypatch)
    cfg = getattr(pkg, cfgname)
    S, T = 3, 4
    n = S * T
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8)
    with pytest.raises(AssertionError) as e:
        dev.he_decode_streams(cfg, torch.zeros(n * pkg.CORE_CH[cfg] * 1024), u8(n * pkg.CORE_CH[cfg] * pkg.ICS_DT.itemsize),
                              u8(n * pkg.SBR_FRAME_DT.itemsize), u8(pkg.SBR_HDR_DT.itemsize),
                              u8(n * pkg.PS_FRAME_DT.itemsize) if cfg == pkg.CFG_HEV2 else None,
                              torch.zeros(S * pkg.STATE_WORDS[cfg]), T, hold=_bad_holds(S, T)[bad])
    assert "hold" in str(e.value)


@pytest.mark.parametrize("bad", ["element", "frame", "dtype", "bool"])
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_wrapper_rejects_a_wrong_hold(pkg, monkeypatch, channels, bad):
    import torch
    dev = _no_device(pkg, monkeypatch)
    S, T = 3, 4
    n = S * T
    with pytest.raises(AssertionError) as e:
        dev.spectral_tools_streams(channels, torch.zeros(n * channels * 1024),
                                   torch.zeros(n * pkg.TOOLS_FRAME_DT.itemsize, dtype=torch.uint8), T,
                                   rng=torch.zeros(S, dtype=torch.int32), hold=_bad_holds(S, T)[bad])
    assert "hold" in str(e.value)


def _create_streams(pkg):
    f = pkg.lib().heaac_pipeline_create_streams
    return f


def _cfg(pkg, sampling_index=3):
    cfg = pkg.AacConfig()
    cfg.object_type, cfg.sampling_index, cfg.sample_rate, cfg.chan_config = 2, sampling_index, 48000, 2
    return cfg


def test_pipeline_create_streams_argument_errors(pkg):
    """T = 0 and every argument error heaac_pipeline_create names come back before a device is looked for"""
    f = _create_streams(pkg)
    h = C.c_void_p()
    good = _cfg(pkg)
    assert f(C.byref(h), C.byref(good), pkg.CFG_LC_STEREO, 4, 0, 1) == HEAAC_ERR_ARG           # T = 0
    assert f(None, C.byref(good), pkg.CFG_LC_STEREO, 4, 2, 1) == HEAAC_ERR_ARG                 # no out
    assert f(C.byref(h), None, pkg.CFG_LC_STEREO, 4, 2, 1) == HEAAC_ERR_ARG                    # no configuration
    assert f(C.byref(h), C.byref(good), pkg.CFG_LC_STEREO, 0, 2, 1) == HEAAC_ERR_ARG           # no streams
    assert f(C.byref(h), C.byref(good), 99, 4, 2, 1) == HEAAC_ERR_ARG                          # no such configuration
    for si in (-1, 13):
        bad = _cfg(pkg, si)
        assert f(C.byref(h), C.byref(bad), pkg.CFG_LC_STEREO, 4, 2, 1) == HEAAC_ERR_ARG        # sampling index
    assert f(C.byref(h), C.byref(good), pkg.CFG_LC_STEREO, 2 ** 40, 2 ** 40, 1) == HEAAC_ERR_ARG   # n T overflows
    assert not h.value


def test_pipeline_create_streams_device_or_not(pkg):
    """without a device: HEAAC_ERR_NODEVICE and no handle; with one: a pipeline that reports its frames per tick"""
    import torch
    f = _create_streams(pkg)
    g = pkg.lib().heaac_pipeline_frames_per_tick
    assert g(None) == 0
    good = _cfg(pkg)
    for T in (1, 2, 8):
        h = C.c_void_p()
        rc = f(C.byref(h), C.byref(good), pkg.CFG_LC_STEREO, 4, T, 1)
        if torch.cuda.is_available():
            assert rc == 0 and h.value and g(h) == T
            pkg.lib().heaac_pipeline_destroy(h)
        else:
            assert rc == HEAAC_ERR_NODEVICE and not h.value


def test_python_pipeline_refuses_no_frames_per_tick(pkg):
    with pytest.raises(pkg.HeaacError) as e:
        pkg.Pipeline(_cfg(pkg), pkg.CFG_LC_STEREO, 4, threads=1, frames_per_tick=0)
    assert "heaac_pipeline_create_streams" in str(e.value)

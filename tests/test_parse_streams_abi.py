"""heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams without a GPU: the calls and the host forms of their
chains are declared with the signatures written out below and exported, a NULL device and bad arguments are
refused before any launch, and the Python wrappers check every tensor's length before anything reaches the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1

AAC_ARGS = ["HeaacDevice *dev", "const HeaacAacConfig *cfg", "HeaacAacStream *d_st", "const uint8_t *d_au",
            "const uint32_t *d_au_offset", "size_t n_streams", "size_t frames_per_stream", "int coeff_channels", "float *d_coeffs",
            "HeaacIcs *d_ics", "HeaacToolsFrame *d_tools", "HeaacAacFrameInfo *d_info", "int32_t *d_status", "uint32_t *d_taken",
            "uint8_t *d_hold", "void *stream"]
HE_ARGS = AAC_ARGS[:3] + ["const HeaacSbrStream *d_sst_in", "HeaacSbrStream *d_sst_out"] + AAC_ARGS[3:12] + [
    "const HeaacSbrHeader *d_hdr", "size_t n_hdr", "HeaacSbrFrame *d_sbr", "HeaacPsFrame *d_ps"] + AAC_ARGS[12:]


def _cfg(pkg):
    c = pkg.AacConfig()
    c.object_type, c.sampling_index, c.sample_rate, c.chan_config = 2, 3, 48000, 2
    return c


def _declared(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, name
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in body.split(",")]


def test_entry_points_declared_with_their_signatures_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_parse.h")).read()
    assert _declared(txt, "heaac_aac_parse_device_streams") == AAC_ARGS
    assert _declared(txt, "heaac_heaac_parse_device_streams") == HE_ARGS
    dbg = open(os.path.join(ROOT, "include", "heaac_debug.h")).read()
    host = lambda args: [a.replace("*d_", "*") for a in args[1:-1]] + ["int32_t *why"]
    assert _declared(dbg, "heaac_debug_aac_parse_core_streams") == host(AAC_ARGS)
    assert _declared(dbg, "heaac_debug_heaac_parse_core_streams") == host(HE_ARGS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("heaac_aac_parse_device_streams", "heaac_heaac_parse_device_streams", "heaac_debug_aac_parse_core_streams",
                 "heaac_debug_heaac_parse_core_streams"):
        assert name in pkg.EXPORTED and name in syms, name
    assert hasattr(pkg.Device, "aac_parse_streams") and hasattr(pkg.Device, "heaac_parse_device_streams")


def test_null_device_and_bad_arguments_are_refused_before_any_launch(pkg):
    f = pkg.lib().heaac_aac_parse_device_streams
    g = pkg.lib().heaac_heaac_parse_device_streams
    cfg = _cfg(pkg)
    d = C.c_void_p(64)
    for S in (0, 1, 4096):
        for T in (0, 1, 3):
            for cc in (1, 2):
                assert f(None, C.byref(cfg), d, d, d, S, T, cc, d, d, d, d, d, d, d, None) == HEAAC_ERR_ARG
                assert g(None, C.byref(cfg), d, d, d, d, d, S, T, cc, d, d, d, d, d, 4, d, d, d, d, d, None) == HEAAC_ERR_ARG
    # with a context that is never dereferenced for these: the configuration, coeff_channels and T == 0 come first
    fake = C.c_void_p(4096)
    for bad in ("cfg", "aot", "si", "cc0", "cc3", "T0"):
        c, cc, T = _cfg(pkg), 2, 2
        if bad == "aot":
            c.object_type = 5
        elif bad == "si":
            c.sampling_index = 13
        elif bad in ("cc0", "cc3"):
            cc = 0 if bad == "cc0" else 3
        elif bad == "T0":
            T = 0
        cp = None if bad == "cfg" else C.byref(c)
        assert f(fake, cp, d, d, d, 1, T, cc, d, d, d, d, d, d, d, None) == HEAAC_ERR_ARG, bad
        assert g(fake, cp, d, d, d, d, d, 1, T, cc, d, d, d, d, d, 4, d, d, d, d, d, None) == HEAAC_ERR_ARG, bad
        assert f(fake, cp, d, d, d, 0, T, cc, d, d, d, d, d, d, d, None) == HEAAC_ERR_ARG, bad       # even with no streams
    assert f(fake, C.byref(cfg), None, None, None, 0, 1, 2, None, None, None, None, None, None, None, None) == 0
    assert g(fake, C.byref(cfg), None, None, None, None, None, 0, 1, 2, None, None, None, None, None, 0, None, None, None, None, None, None) == 0
    # NULL and misaligned pointers, an S * T that overflows or lies beyond the unit index, overlapping states, n_hdr == 0
    a16, other = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    good_f = [fake, C.byref(cfg), d, d, d, 8, 3, 2, a16, d, d, d, d, d, d, None]
    for k in (2, 3, 4, 8, 9, 10, 11, 12, 13):
        bad = list(good_f)
        bad[k] = None
        assert f(*bad) == HEAAC_ERR_ARG, k
    for k in (4, 8, 10, 11, 12, 13):
        bad = list(good_f)
        bad[k] = C.c_void_p(good_f[k].value + 2)
        assert f(*bad) == HEAAC_ERR_ARG, k
    for S, T in ((1 << 40, 1 << 40), (1 << 20, 1 << 13), (1 << 62, 4), (8, 1 << 31), ((1 << 31) * 64, 1)):
        bad = list(good_f)
        bad[5], bad[6] = S, T
        assert f(*bad) == HEAAC_ERR_ARG, (S, T)
    good_g = [fake, C.byref(cfg), d, a16, other, d, d, 8, 3, 2, a16, d, d, d, d, 4, d, d, d, d, d, None]
    for k in (2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 16, 18, 19):
        bad = list(good_g)
        bad[k] = None
        assert g(*bad) == HEAAC_ERR_ARG, k
    for k in (3, 4, 6, 10, 12, 13, 14, 16, 18, 19):
        bad = list(good_g)
        bad[k] = C.c_void_p(good_g[k].value + 2)
        assert g(*bad) == HEAAC_ERR_ARG, k
    bad = list(good_g)
    bad[15] = 0
    assert g(*bad) == HEAAC_ERR_ARG
    bad = list(good_g)
    bad[4] = C.c_void_p(a16.value + 3336 * 7)                          # the last row of one array is the first of the other
    assert g(*bad) == HEAAC_ERR_ARG
    mono = _cfg(pkg)
    mono.chan_config, mono.sbr, mono.ps = 1, 1, 1
    bad = list(good_g)
    bad[1], bad[17] = C.byref(mono), None                               # Parametric Stereo without a PS array
    assert g(*bad) == HEAAC_ERR_ARG


class _NoDevice:
    """Stands in for the library: the wrapper must not get as far as calling it."""
    def __getattr__(self, name):
        raise AssertionError("device call %s reached" % name)


def _tensors(pkg, S, T, cc):
    import torch
    n = S * T
    return dict(streams=torch.zeros(S * pkg.AAC_STREAM_DT.itemsize, dtype=torch.uint8),
                coeffs=torch.zeros(n * cc * 1024, dtype=torch.float32),
                ics=torch.zeros(n * cc * pkg.ICS_DT.itemsize, dtype=torch.uint8),
                tools=torch.zeros(n * pkg.TOOLS_FRAME_DT.itemsize, dtype=torch.uint8),
                info=torch.zeros(n * pkg.AAC_INFO_DT.itemsize, dtype=torch.uint8),
                status=torch.zeros(n, dtype=torch.int32), taken=torch.zeros(S, dtype=torch.int32),
                hold=torch.zeros(n, dtype=torch.uint8))


@pytest.mark.parametrize("which", ["streams", "coeffs", "ics", "tools", "info", "status", "taken", "hold"])
def test_wrapper_rejects_wrong_lengths(pkg, monkeypatch, which):
    import torch
    monkeypatch.setattr(pkg, "lib", lambda: _NoDevice())
    dev = pkg.Device.__new__(pkg.Device)
    dev._h = C.c_void_p()
    S, T, cc = 5, 3, 2
    a = _tensors(pkg, S, T, cc)
    a[which] = a[which][:-1]
    au = torch.zeros(400, dtype=torch.uint8)
    off = torch.from_numpy((np.arange(S * T + 1) * 20).astype(np.int32))
    with pytest.raises(AssertionError) as e:
        dev.aac_parse_streams(_cfg(pkg), a.pop("streams"), au, off, T, coeff_channels=cc, **a)
    assert which in str(e.value)
    a = _tensors(pkg, S, T, cc)
    for bad_T, what in ((0, "frames_per_stream"), (2, "au_offset")):          # 15 units are no whole number of pairs
        with pytest.raises(AssertionError) as e:
            dev.aac_parse_streams(_cfg(pkg), a["streams"], au, off, bad_T, coeff_channels=cc)
        assert what in str(e.value)

"""heaac_sbr_parse_device and heaac_heaac_parse_device without a GPU: the calls and the host form of the walk are
declared and exported, a NULL device is refused, and what the calls refuse before any launch -- a NULL array, state
arrays that overlap, n_hdr = 0, a mono PS configuration without d_ps, a misaligned pointer -- is refused by the host
form, which goes through the same check; n = 0 is HEAAC_OK whatever the arrays are."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import sbr_device_common as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAAC_ERR_ARG = -1


def test_sbr_parse_device_entry_points_declared_and_exported(pkg):
    txt = open(os.path.join(ROOT, "include", "heaac_parse.h")).read()
    assert re.search(r"\bint\s+heaac_sbr_parse_device\s*\(", txt)
    assert re.search(r"\bint\s+heaac_heaac_parse_device\s*\(", txt)
    dbg = open(os.path.join(ROOT, "include", "heaac_debug.h")).read()
    assert re.search(r"\bint\s+heaac_debug_sbr_parse_core\s*\(", dbg)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("heaac_sbr_parse_device", "heaac_heaac_parse_device", "heaac_debug_sbr_parse_core"):
        assert name in pkg.EXPORTED and name in syms, name
    assert hasattr(pkg.Device, "sbr_parse_device") and hasattr(pkg.Device, "heaac_parse_device")
    assert pkg.PARSE_DEFERRED == pkg.PARSE_NO_SBR == 1              # why a unit without a payload comes back OK


def _host_args(pkg, n=2, cpe=False):
    cfg = SD.he_cfg(pkg, cpe)
    a = dict(cfg=cfg, sst_in=pkg.sbr_streams(n), sst_out=pkg.sbr_streams(n), au=np.zeros(64, np.uint8),
             off=np.arange(n + 1, dtype=np.uint32) * 8, info=np.zeros(n, pkg.AAC_INFO_DT), aac=np.ones(n, np.int32),
             hdr=np.zeros(1, pkg.SBR_HDR_DT), sbr=np.zeros(n, pkg.SBR_FRAME_DT), ps=np.zeros(n, pkg.PS_FRAME_DT),
             status=np.full(n, 7, np.int32), why=np.zeros(n, np.int32))
    return a


def _call(pkg, a, n, n_hdr=1, **over):
    g = pkg.lib().heaac_debug_sbr_parse_core
    p = {k: (C.addressof(v) if k == "cfg" else v.ctypes.data) for k, v in a.items()}
    p.update(over)
    return g(p["cfg"], p["sst_in"], p["sst_out"], p["au"], p["off"], p["info"], p["aac"], n, p["hdr"], n_hdr, p["sbr"], p["ps"],
             p["status"], p["why"])


def test_what_the_calls_refuse_before_they_look_at_a_unit(pkg):
    n = 2
    a = _host_args(pkg, n)
    assert _call(pkg, a, n) == 0 and list(a["status"]) == [pkg.PARSE_DEFERRED] * n      # (AAC status not OK: nothing is read)
    assert np.array_equal(a["sst_out"], a["sst_in"])
    for k in ("cfg", "sst_in", "sst_out", "au", "off", "info", "hdr", "sbr", "status"):
        assert _call(pkg, a, n, **{k: None}) == HEAAC_ERR_ARG, k
    assert _call(pkg, a, n, aac=None, why=None) == 0                                       # the two optional ones
    assert _call(pkg, a, n, n_hdr=0) == HEAAC_ERR_ARG
    # state arrays that are the same, or that overlap by a row
    assert _call(pkg, a, n, sst_out=a["sst_in"].ctypes.data) == HEAAC_ERR_ARG
    three = pkg.sbr_streams(n + 1)
    assert _call(pkg, a, n, sst_in=three.ctypes.data, sst_out=three[1:].ctypes.data) == HEAAC_ERR_ARG
    assert _call(pkg, a, n, sst_in=three[1:].ctypes.data, sst_out=three.ctypes.data) == HEAAC_ERR_ARG
    assert _call(pkg, a, 1, sst_in=three.ctypes.data, sst_out=three[1:].ctypes.data) == 0    # side by side is fine
    # Parametric Stereo asked for on a mono configuration, and nowhere to put it
    assert _call(pkg, a, n, ps=None) == HEAAC_ERR_ARG
    stereo = _host_args(pkg, n, cpe=True)
    assert _call(pkg, stereo, n, ps=None) == 0
    mono_no_ps = _host_args(pkg, n)
    mono_no_ps["cfg"].ps = 0
    assert _call(pkg, mono_no_ps, n, ps=None) == 0
    # records are read and written in words
    assert _call(pkg, a, n, sbr=a["sbr"].ctypes.data + 2) == HEAAC_ERR_ARG
    # n = 0: nothing is looked at
    assert _call(pkg, a, 0, n_hdr=0, **{k: None for k in a if k != "cfg"}) == 0
    assert _call(pkg, a, 0, cfg=None) == HEAAC_ERR_ARG


def test_a_null_device_is_refused(pkg):
    cfg = SD.he_cfg(pkg, False)
    d = C.c_void_p(64)
    f = pkg.lib().heaac_sbr_parse_device
    g = pkg.lib().heaac_heaac_parse_device
    for n in (0, 1, 4096):
        assert f(None, C.byref(cfg), d, d, d, d, d, d, n, d, 1, d, d, d, None) == HEAAC_ERR_ARG
        assert g(None, C.byref(cfg), d, d, d, d, d, n, 1, d, d, d, d, d, 1, d, d, d, None) == HEAAC_ERR_ARG

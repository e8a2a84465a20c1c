"""The C-ABI library loads on a machine without a GPU and exports every symbol that
include/*.h declares (no compute calls here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = set()
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if not h.endswith(".h") or h == "heaac_iso_tables.h":        # (constant tables, no entry points)
            continue
        txt = open(os.path.join(ROOT, "include", h)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        for m in re.finditer(r"^\s*(?:extern\s+)?[A-Za-z_][\w\s\*]*?\b((?:heaac|ff|av)_\w+)\s*(?:\(|\[|;)", txt, re.M):
            names.add(m.group(1))
    return names


def test_headers_declare_what_the_package_lists(pkg):
    decl = declared_symbols()
    assert set(pkg.EXPORTED) <= decl - {"av_class"}, set(pkg.EXPORTED) - decl
    # nothing declared is missing from the package's list either
    assert decl - {"heaac_iso_qmf_c", "heaac_iso_noise", "av_class"} <= set(pkg.EXPORTED), decl - set(pkg.EXPORTED)   # av_class: a field of the AVCodecContext layout


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    missing = [s for s in pkg.EXPORTED if s not in exported]
    assert not missing, missing
    for s in pkg.EXPORTED:
        getattr(lib, s)


def test_record_sizes_match_header(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "heaac_dsp.h"\n#include "heaac_fft.h"\n#include "heaac_codec.h"\n#include <stdio.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n",sizeof(HeaacIcs),sizeof(HeaacSbrHeader),'
                   'sizeof(HeaacSbrChannel),sizeof(HeaacSbrFrame),sizeof(HeaacPsFrame),HEAAC_ST_SBR,HEAAC_ST_PS,'
                   'HEAAC_STATE_WORDS_HEV1,HEAAC_STATE_WORDS_HEV2,HEAAC_STATE_WORDS_HEV1_MONO);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert v[:5] == [pkg.ICS_DT.itemsize, pkg.SBR_HDR_DT.itemsize, pkg.SBR_CH_DT.itemsize,
                     pkg.SBR_FRAME_DT.itemsize, pkg.PS_FRAME_DT.itemsize]
    assert v[5:] == [pkg.ST_SBR, pkg.ST_PS, pkg.STATE_WORDS[pkg.CFG_HEV1], pkg.STATE_WORDS[pkg.CFG_HEV2],
                     pkg.STATE_WORDS[pkg.CFG_HEV1_MONO]]


def test_no_gpu_means_loud_failure(pkg):
    """Without a HIP device the product must refuse, not fall back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = pkg.lib().heaac_device_create(C.byref(h), C.c_size_t(16))
    assert rc in (-4, -2) and not h.value
    with pytest.raises(pkg.HeaacError):
        pkg.Device()
    ctx = (C.c_char * 256)()
    assert pkg.lib().ff_mdct_init(ctx, 11, 1, C.c_double(1.0)) == -1


def test_debug_xbands_checks_its_arguments(pkg):
    """include/heaac_debug.h: a NULL context or buffer is HEAAC_ERR_ARG before anything touches the device (the bound
    on n_frames needs a device: tests/test_streams_gpu.py)."""
    lib = pkg.lib()
    buf = (C.c_uint8 * 16)()
    assert lib.heaac_debug_xbands(None, buf, C.c_size_t(8)) == -1
    assert lib.heaac_debug_xbands(None, None, C.c_size_t(0)) == -1
    h = C.c_void_p()
    if lib.heaac_device_create(C.byref(h), C.c_size_t(64)) == 0:
        try:
            assert lib.heaac_debug_xbands(h, None, C.c_size_t(8)) == -1
            assert lib.heaac_debug_xbands(h, buf, C.c_size_t(65)) == -1          # past the one chunk of 64 frames
            assert lib.heaac_debug_xbands(h, buf, C.c_size_t(8)) == 0
        finally:
            lib.heaac_device_destroy(h)
    else:
        assert not h.value


def test_product_does_not_reference_oracle():
    """oracle/ is test infrastructure: nothing under the package may include or link it."""
    bad = []
    for dp, _, files in os.walk(os.path.join(ROOT, "ffmpeg-heaac_amd")):
        if "_obj" in dp or "__pycache__" in dp:
            continue
        for f in files:
            if f.endswith((".so", ".o", ".pyc")):
                continue
            txt = open(os.path.join(dp, f), errors="ignore").read()
            if re.search(r"oracle\.h|oracle_lib|liboracle|libheaac_oracle|oracle/", txt):
                bad.append(os.path.join(dp, f))
    assert not bad, bad
    ldd = subprocess.check_output(["ldd", os.path.join(ROOT, "ffmpeg-heaac_amd", "libheaac_amd.so")]).decode()
    assert "oracle" not in ldd


def test_sbr_header_product_matches_oracle(pkg, oracle):
    """heaac_sbr_make_header vs the oracle's independent restatement over a grid of headers
    (also pins the survey's probe: k0=13 kx=13 m=32 n_master=16 n_high=16 n_low=8 n_q=4
    n_lim=4 patches=3, measured on the real reference -- SURVEY.md s8c)."""
    h = pkg.sbr_make_header()[0]
    assert (h["k0"], h["k2"], h["kx"], h["m"], h["n_master"], h["n"][1], h["n"][0], h["n_q"], h["n_lim"],
            h["num_patches"]) == (13, 45, 13, 32, 16, 16, 8, 4, 4, 3)
    rng = np.random.default_rng(0)
    ok = 0
    for _ in range(1500):
        args = (int(rng.choice([48000, 44100, 32000, 24000])), int(rng.integers(0, 16)), int(rng.integers(0, 16)),
                int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 2)), int(rng.integers(0, 4)),
                int(rng.integers(0, 4)))
        try:
            a = pkg.sbr_make_header(*args)[0]
        except ValueError:
            a = None
        try:
            b = oracle.sbr_make_header(*args)[0]
        except ValueError:
            b = None
        assert (a is None) == (b is None), args
        if a is None:
            continue
        ok += 1
        for f in ("k0", "k2", "kx", "m", "n", "n_q", "n_lim", "n_master", "num_patches"):
            assert np.array_equal(a[f], b[f]), (args, f)
        for f, c in (("patch_num_subbands", a["num_patches"]), ("patch_start_subband", a["num_patches"]),
                     ("f_tablelow", a["n"][0] + 1), ("f_tablehigh", a["n"][1] + 1),
                     ("f_tablenoise", a["n_q"] + 1), ("f_tablelim", a["n_lim"] + 1)):
            assert np.array_equal(a[f][:c], b[f][:c]), (args, f)
    assert ok > 300

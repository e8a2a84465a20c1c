"""heaac_pipeline_create_ex and the host steps of a device-parse tick that need no device: the argument checks, the
loud failure without a GPU, and pack / stop list (csrc/pipeline_pack.h) through their debug exports and, stand-alone
under ASan / UBSan, through tests/c/pipeline_pack.c."""
import ctypes as C
import os
import subprocess

import numpy as np

import test_parse as TP
import test_sbr_parse as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg-heaac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")


def test_create_ex_checks_arguments_and_fails_loudly_without_a_device(pkg):
    import torch
    lib = pkg.lib()
    h = C.c_void_p(1)
    cfg = TS._he_cfg(pkg, 1, True)
    DP = pkg.PIPELINE_DEVICE_PARSE
    assert DP == 1
    ex = lambda c, he, n, T, flags: lib.heaac_pipeline_create_ex(C.byref(h), C.byref(c) if c is not None else None, he,
                                                                 C.c_size_t(n), C.c_size_t(T), 1, flags)
    for flags in (0, DP):
        h.value = 1
        assert ex(cfg, 99, 4, 2, flags) == -1 and not h.value
        assert ex(None, pkg.CFG_HEV2, 4, 2, flags) == -1
        assert ex(cfg, pkg.CFG_HEV2, 0, 2, flags) == -1
        assert ex(cfg, pkg.CFG_HEV2, 4, 0, flags) == -1
    assert lib.heaac_pipeline_create_ex(None, C.byref(cfg), pkg.CFG_HEV2, C.c_size_t(4), C.c_size_t(1), 1, DP) == -1
    # unknown flag bits, alone and next to the known one
    for flags in (2, 3, 1 << 30, -1):
        h.value = 1
        assert ex(cfg, pkg.CFG_HEV2, 4, 1, flags) == -1 and not h.value
    # an object type the device parser refuses: only with the flag
    ltp = TP._cfg(pkg, 2, 3, 1)
    ltp.object_type = 4
    h.value = 1
    assert ex(ltp, pkg.CFG_LC_MONO, 4, 1, DP) == -1 and not h.value
    # beyond the walk's 32-bit unit index
    assert ex(cfg, pkg.CFG_HEV2, 1 << 20, 1 << 13, DP) == -1
    # a mono configuration that signals PS has no PS records under HEAAC_CFG_HEV1_MONO
    assert cfg.ps != 0 and cfg.chan_config == 1
    assert ex(cfg, pkg.CFG_HEV1_MONO, 4, 1, DP) == -1
    if not torch.cuda.is_available():
        for flags in (0, DP):
            h.value = 1
            assert ex(cfg, pkg.CFG_HEV2, 4, 2, flags) == -4 and not h.value
        assert ex(ltp, pkg.CFG_LC_MONO, 4, 1, 0) == -4           # flags = 0 is heaac_pipeline_create_streams
        try:
            pkg.Pipeline(cfg, pkg.CFG_HEV2, 4, threads=1, frames_per_tick=2, device_parse=True)
        except pkg.HeaacError:
            pass
        else:
            raise AssertionError("Pipeline(device_parse=True) without a device")
    # the counts of no pipeline
    c = (C.c_ulonglong * 2)(7, 7)
    lib.heaac_pipeline_parse_counts(None, c)
    assert list(c) == [0, 0]


def _pack(pkg, aus, sizes=None, with_bytes=True):
    n = len(aus)
    keep = [C.create_string_buffer(bytes(a), len(a)) for a in aus]
    ptrs = (C.c_char_p * n)(*[C.cast(k, C.c_char_p) for k in keep])
    sizes = (C.c_int * n)(*(sizes if sizes is not None else [len(a) for a in aus]))
    off = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    total = sum(max(0, s) for s in sizes)
    buf = np.full(total + 8, 0xA5, np.uint8)                      # 8 guard bytes behind the tick's
    rc = pkg.lib().heaac_debug_pipeline_pack(ptrs, sizes, n, buf.ctypes.data_as(C.c_void_p) if with_bytes else None,
                                             off.ctypes.data_as(C.c_void_p))
    return rc, off, buf, total


def test_pack_lays_units_end_to_end_and_empty_units_take_no_bytes(pkg):
    rng = np.random.default_rng(5)
    aus = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in (3, 0, 700, 1, 0, 0, 17)]
    sizes = [len(a) for a in aus]
    sizes[4] = -5                                                  # size < 0: an empty unit as well
    rc, off, buf, total = _pack(pkg, aus, sizes)
    assert rc == 0 and total == 3 + 700 + 1 + 17
    want = np.concatenate([[0], np.cumsum([max(0, s) for s in sizes])])
    assert np.array_equal(off.astype(np.int64), want)
    assert off[1] == off[2] and off[4] == off[5] == off[6]          # the empty and the negative ones
    for i, a in enumerate(aus):
        assert bytes(buf[off[i]:off[i + 1]]) == (a if sizes[i] > 0 else b"")
    assert (buf[total:] == 0xA5).all()
    # a tick of nothing but empty units: every offset 0, not a byte written; NULL pointers are not looked at
    n = 6
    sizes = (C.c_int * n)(0, -1, 0, 0, -7, 0)
    ptrs = (C.c_char_p * n)()
    off = np.full(n + 1, 7, np.uint32)
    buf = np.full(8, 0xA5, np.uint8)
    assert pkg.lib().heaac_debug_pipeline_pack(ptrs, sizes, n, buf.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p)) == 0
    assert not off.any() and (buf == 0xA5).all()
    # no units at all
    off = np.full(1, 7, np.uint32)
    assert pkg.lib().heaac_debug_pipeline_pack(None, (C.c_int * 1)(), 0, None, off.ctypes.data_as(C.c_void_p)) == 0 and off[0] == 0


def test_a_tick_beyond_32_bit_offsets_is_refused_from_the_sizes_alone(pkg):
    f = pkg.lib().heaac_debug_pipeline_pack
    off = np.zeros(4, np.uint32)
    po = off.ctypes.data_as(C.c_void_p)
    big = 0x7fffffff
    assert f(None, (C.c_int * 3)(big, big, 1), 3, None, po) == 0 and int(off[3]) == 0xffffffff     # the largest tick
    assert f(None, (C.c_int * 3)(big, big, 2), 3, None, po) == -1                                  # 4 GiB
    assert f(None, (C.c_int * 3)(big, big, big), 3, None, po) == -1
    assert f(None, (C.c_int * 3)(big, -big, big), 3, None, po) == 0 and int(off[3]) == 2 * big     # an empty unit in between
    # bytes asked for without units to read them from, and no size / offset array
    assert f(None, (C.c_int * 1)(4), 1, po, po) == -1
    assert f(None, None, 1, None, po) == -1 and f(None, (C.c_int * 1)(4), 1, None, None) == -1


def test_stop_list_names_the_stopped_streams_and_where_their_units_are_staged(pkg):
    f = pkg.lib().heaac_debug_pipeline_stops
    rng = np.random.default_rng(11)
    for n, T in ((1, 1), (7, 1), (7, 5), (130, 3), (64, 2)):
        for fill in ("mixed", "none", "all"):
            taken = rng.integers(0, T + 1, n).astype(np.uint32)
            if fill == "none":
                taken[:] = T
            if fill == "all":
                taken[:] = 0
            lst, base = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n + 1, 0xA5A5A5A5, np.uint32)
            m = f(taken.ctypes.data_as(C.c_void_p), n, T, lst.ctypes.data_as(C.c_void_p), base.ctypes.data_as(C.c_void_p))
            want = np.flatnonzero(taken < T)
            assert m == want.size and np.array_equal(lst[:m], want)
            rest = T - taken[want].astype(np.int64)
            assert np.array_equal(base[:m + 1].astype(np.int64), np.concatenate([[0], np.cumsum(rest)]))
            assert (lst[m:] == 0xA5A5A5A5).all() and (base[m + 1:] == 0xA5A5A5A5).all()


def test_pack_and_stop_list_under_sanitizers_with_every_unit_at_the_end_of_its_block(pkg):
    """tests/c/pipeline_pack.c: a stand-alone program over csrc/pipeline_pack.h, built with ASan / UBSan and run as a
    child -- every unit ends where its heap block ends, the packed buffer holds exactly the tick's bytes, the list and
    base arrays exactly n and n + 1 entries."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "pipeline_pack")
    deps = [os.path.join(ROOT, "tests", "c", "pipeline_pack.c"), os.path.join(CSRC, "pipeline_pack.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wall", "-Werror", "-I", CSRC, deps[0], "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode(), out.stderr.decode()[-2000:])
    assert b"rounds ok" in out.stdout

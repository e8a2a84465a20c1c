"""ffmpeg-heaac_amd -- MI355X-native HE-AAC decode DSP (host-side Python mirror).

The product is the C-ABI shared library `libheaac_amd.so` (include/heaac_dsp.h,
include/heaac_fft.h, include/heaac_codec.h): hand-written HIP kernels for
gfx950 plus C host code.  This module only binds it with ctypes so that tests
and bench.py can drive it; PyTorch supplies device memory and streams, nothing
else.  There is NO CPU fallback: if the library is missing, or no gfx950 device
is visible when a compute entry point is called, an exception is raised.

The directory name contains a hyphen; load it with
    import importlib.util  (see __graft_entry__.load_package)
or simply `from __graft_entry__ import load_package; heaac = load_package()`.
"""
import ctypes as C
import os

import numpy as np

from . import prototypes

_HERE = os.path.dirname(os.path.abspath(__file__))
# HEAAC_LIB_PATH: measurement tooling (tools/abv.sh) points the binding at a variant build under ab/
# without touching the product library; unset everywhere else.  Never silently: the override is announced on
# stderr when the library is loaded, LIB_OVERRIDDEN says so to whoever reports numbers (bench.py prints it).
PRODUCT_LIB_PATH = os.path.join(_HERE, "libheaac_amd.so")
LIB_PATH = os.environ.get("HEAAC_LIB_PATH") or PRODUCT_LIB_PATH
LIB_OVERRIDDEN = os.path.realpath(LIB_PATH) != os.path.realpath(PRODUCT_LIB_PATH)

# ---- constants (include/heaac_dsp.h) ----
ONLY_LONG_SEQUENCE, LONG_START_SEQUENCE, EIGHT_SHORT_SEQUENCE, LONG_STOP_SEQUENCE = 0, 1, 2, 3
CFG_LC_MONO, CFG_LC_STEREO, CFG_HEV1, CFG_HEV2, CFG_HEV1_MONO = 0, 1, 2, 3, 4
PCM_F32, PCM_S16, PCM_S16_SSE2 = 0, 1, 2
ADD_BIAS = 385.0

ST_SAVED, ST_SBR, ST_SYNTH, ST_PS = 512, 1972, 1152, 4500
STATE_WORDS = {
    CFG_LC_MONO: ST_SAVED,
    CFG_LC_STEREO: 2 * ST_SAVED,
    CFG_HEV1: 2 * ST_SAVED + 2 * ST_SBR + 2 * ST_SYNTH,
    CFG_HEV1_MONO: ST_SAVED + ST_SBR + ST_SYNTH,
    CFG_HEV2: ST_SAVED + ST_SBR + 2 * ST_SYNTH + ST_PS,
}
CORE_CH = {CFG_LC_MONO: 1, CFG_LC_STEREO: 2, CFG_HEV1: 2, CFG_HEV2: 1, CFG_HEV1_MONO: 1}
OUT_CH = {CFG_LC_MONO: 1, CFG_LC_STEREO: 2, CFG_HEV1: 2, CFG_HEV2: 2, CFG_HEV1_MONO: 1}
OUT_LEN = {CFG_LC_MONO: 1024, CFG_LC_STEREO: 1024, CFG_HEV1: 2048, CFG_HEV2: 2048, CFG_HEV1_MONO: 2048}

# Algorithmic HBM bytes per frame, SURVEY.md s8(d) / BASELINE.md s3 (f32 PCM out).
ALGO_BYTES = {CFG_LC_STEREO: 24584, CFG_HEV1: 83976, CFG_HEV2: 85284}

# ---- record dtypes (include/heaac_dsp.h) ----
ICS_DT = np.dtype([("window_sequence", "u1", (2,)), ("use_kb_window", "u1", (2,))])
SBR_HDR_DT = np.dtype([
    ("k0", "u1"), ("k2", "u1"), ("kx", "u1"), ("m", "u1"),
    ("n", "u1", (2,)), ("n_q", "u1"), ("n_lim", "u1"),
    ("n_master", "u1"), ("num_patches", "u1"), ("bs_limiter_gains", "u1"),
    ("bs_interpol_freq", "u1"), ("bs_smoothing_mode", "u1"), ("bs_amp_res_header", "u1"),
    ("pad0", "u1", (2,)),
    ("patch_num_subbands", "u1", (6,)), ("patch_start_subband", "u1", (6,)),
    ("f_tablenoise", "u1", (6,)), ("pad1", "u1", (2,)),
    ("f_tablelow", "u1", (28,)), ("f_tablehigh", "u1", (52,)), ("f_tablelim", "u1", (32,)),
    ("map_hi", "u1", (64,)), ("map_lo", "u1", (64,)), ("map_nq", "u1", (64,)),
    ("map_lim", "u1", (64,)), ("map_mid", "u1", (64,)), ("map_src", "u1", (64,)),
])
SBR_CH_DT = np.dtype([
    ("bs_num_env", "u1"), ("bs_num_noise", "u1"), ("bs_amp_res", "u1"), ("bs_add_harmonic_flag", "u1"),
    ("bs_freq_res", "u1", (8,)), ("t_env", "u1", (8,)), ("t_q", "u1", (3,)),
    ("t_env_num_env_old", "u1"), ("e_a", "i1", (2,)),
    ("bs_invf_mode", "u1", (2, 5)), ("bs_add_harmonic", "u1", (48,)),
    ("env_facs_q", "u1", (5, 48)), ("noise_facs_q", "u1", (2, 5)), ("pad", "u1", (2,)),
])
SBR_FRAME_DT = np.dtype([
    ("hdr", "<u2"), ("start", "u1"), ("reset", "u1"), ("kx_old", "u1"), ("m_old", "u1"),
    ("bs_coupling", "u1"), ("pad", "u1"), ("ch", SBR_CH_DT, (2,)),
])
PS_FRAME_DT = np.dtype([
    ("start", "u1"), ("is34bands", "u1"), ("is34bands_old", "u1"), ("num_env", "u1"),
    ("num_env_old", "u1"), ("enable_ipdopd", "u1"), ("iid_quant", "u1"), ("icc_mode", "u1"),
    ("nr_iid_par", "u1"), ("nr_icc_par", "u1"), ("nr_ipdopd_par", "u1"), ("pad", "u1"),
    ("border_position", "i1", (8,)),
    ("iid_par", "i1", (5, 34)), ("icc_par", "i1", (5, 34)),
    ("ipd_par", "i1", (5, 17)), ("opd_par", "i1", (5, 17)), ("pad2", "u1", (2,)),
])
TOOLS_ICS_DT = np.dtype([
    ("num_windows", "u1"), ("num_window_groups", "u1"), ("max_sfb", "u1"), ("num_swb", "u1"),
    ("tns_max_bands", "u1"), ("pad", "u1", (3,)), ("group_len", "u1", (8,)), ("swb_offset", "<u2", (64,)),
])
TNS_DT = np.dtype([
    ("present", "u1"), ("n_filt", "u1", (8,)), ("length", "u1", (8, 4)), ("direction", "u1", (8, 4)),
    ("order", "u1", (8, 4)), ("pad", "u1", (3,)), ("coef", "<f4", (8, 4, 20)),
])
PRED_DT = np.dtype([("predictor_present", "u1"), ("predictor_reset_group", "u1"), ("pred_sfb_max", "u1"),
                    ("pad", "u1"), ("prediction_used", "u1", (44,))])
PRED_STATE_DT = np.dtype([("cor0", "<f4"), ("cor1", "<f4"), ("var0", "<f4"), ("var1", "<f4"), ("r0", "<f4"), ("r1", "<f4")])
MAX_PREDICTORS = 672
TOOLS_CH_DT = np.dtype([("ics", TOOLS_ICS_DT), ("band_type", "u1", (128,)), ("sf", "<f4", (128,)), ("tns", TNS_DT),
                        ("pred", PRED_DT)])
TOOLS_FRAME_DT = np.dtype([
    ("common_window", "u1"), ("ms_present", "u1"), ("pad", "u1", (2,)), ("ms_mask", "u1", (128,)),
    ("ch", TOOLS_CH_DT, (2,)),
])
assert TOOLS_ICS_DT.itemsize == 144 and TNS_DT.itemsize == 2668 and TOOLS_FRAME_DT.itemsize == 7132
MAX_CCE, MAX_CCE_LINKS = 16, 4
CC_BEFORE_TNS, CC_BETWEEN_TNS_AND_IMDCT, CC_AFTER_IMDCT = 0, 1, 3
TOOLS_PRE, TOOLS_POST, TOOLS_ALL = 1, 2, 3
CCE_LINK_DT = np.dtype([("target_ch", "u1"), ("pad", "u1", (3,)), ("gain", "<f4", (120,))])
CCE_FRAME_DT = np.dtype([("present", "u1"), ("elem_id", "u1"), ("coupling_point", "u1"), ("n_links", "u1"),
                         ("behind_target", "u1"), ("seq", "u1"), ("outputs_before", "u1"), ("pad", "u1"), ("ics", TOOLS_ICS_DT), ("band_type", "u1", (128,)),
                         ("link", CCE_LINK_DT, (MAX_CCE_LINKS,))])
assert CCE_LINK_DT.itemsize == 484 and CCE_FRAME_DT.itemsize == 2216
assert SBR_HDR_DT.itemsize == 532 and SBR_CH_DT.itemsize == 336
assert SBR_FRAME_DT.itemsize == 680 and PS_FRAME_DT.itemsize == 532

# Every symbol include/*.h declares (checked by tests/test_abi.py): the functions, whose prototypes lib() applies, and
# two data symbols.
EXPORTED = list(prototypes.PROTOTYPES) + ["heaac_aac_decoder", "ff_sine_windows"]


# heaac_dsp.h: first rule a record breaks
BAD_RULES = ["NONE", "HDR_INDEX", "HDR_RANGE", "HDR_COUNTS", "HDR_TABLE", "HDR_MAP", "HDR_FLAGS", "HDR_UNSTARTED",
             "SBR_NUM_ENV", "SBR_T_ENV", "SBR_T_Q", "SBR_FLAGS", "SBR_OLD_RANGE",
             "PS_NUM_ENV", "PS_BORDER", "PS_NR_PAR", "PS_PAR"]


class HeaacError(RuntimeError):
    pass


def validate_frame(cfg, sbr, hdr, ps=None):
    """Host-side record check of ONE frame (numpy records): returns the name of the first rule broken,
    "NONE" if the frame is valid."""
    sbr = np.ascontiguousarray(sbr, dtype=SBR_FRAME_DT).reshape(-1)[:1]
    hdr = np.ascontiguousarray(hdr, dtype=SBR_HDR_DT).reshape(-1)
    if ps is not None:
        ps = np.ascontiguousarray(ps, dtype=PS_FRAME_DT).reshape(-1)[:1]
    r = lib().heaac_validate_frame(cfg, _np(sbr), _np(hdr), hdr.shape[0], _np(ps))
    if r < 0:
        raise HeaacError("heaac_validate_frame: bad call")
    return BAD_RULES[r]


_lib = None


KERNEL_SOURCE_EXTRA = ("kernels.h", "tables.h", "validate.h")


def kernel_source_files():
    """The device sources of the kernels bench.py's workloads launch, relative to the repository root: csrc/k_*.hip,
    csrc/k_*.h, kernels.h, tables.h, validate.h and the record header include/heaac_dsp.h -- without k_tools.hip (the
    spectral tools: no bench workload runs them; tools/tools_rate.py measures them by themselves), k_parse.hip and
    k_parse_streams.hip (the device parsers: tools/parse_rate.py --device)."""
    import glob
    d = os.path.join(_HERE, "csrc")
    files = sorted(f for f in glob.glob(os.path.join(d, "k_*.hip")) + glob.glob(os.path.join(d, "k_*.h"))
                   if os.path.basename(f) not in ("k_tools.hip", "k_parse.hip", "k_parse_streams.hip"))
    files += [os.path.join(d, f) for f in KERNEL_SOURCE_EXTRA]
    files.append(os.path.join(os.path.dirname(_HERE), "include", "heaac_dsp.h"))
    return [os.path.relpath(f, os.path.dirname(_HERE)) for f in files]


def kernel_source_sha(read=None):
    """SHA-256 over the CODE of the device sources (comments and white space do not count; host-side sources --
    parsers, pipelines, the C API -- do not either): a measurement stored under profiles/ is tied to the kernels it was
    taken on, and bench.py refuses a traffic figure whose stamp differs.  read(relative path) -> text lets
    tools/traffic_stamp.py hash the files of another commit."""
    import hashlib
    import re
    root = os.path.dirname(_HERE)
    if read is None:
        read = lambda rel: open(os.path.join(root, rel), encoding="utf-8").read()
    h = hashlib.sha256()
    for rel in kernel_source_files():
        txt = read(rel)
        txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)          # block comments
        txt = re.sub(r"//[^\n]*", " ", txt)                       # line comments (no string literal of these files holds //)
        txt = " ".join(txt.split())
        h.update(os.path.basename(rel).encode())
        h.update(txt.encode())
    return h.hexdigest()[:16]


def lib():
    """Load libheaac_amd.so; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HeaacError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C ffmpeg-heaac_amd/csrc). There is no CPU fallback." % LIB_PATH)
        # PyTorch ships its own HIP runtime.  If this library is loaded first it binds /opt/rocm's copy, torch then
        # brings a second one into the process and whichever initialises later sees no device: load torch first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if LIB_OVERRIDDEN:
            import sys
            print("ffmpeg-heaac_amd: HEAAC_LIB_PATH is set -- using %s instead of the product library" % LIB_PATH,
                  file=sys.stderr)
        _lib = C.CDLL(LIB_PATH)
        prototypes.apply(_lib)
    return _lib


def _check(rc, what):
    if rc != 0:
        raise HeaacError("%s failed: %s (%d)" % (what, lib().heaac_strerror(rc).decode(), rc))


def get_table(name, n=4096):
    """Host-built table by name (for table-parity tests; no GPU needed)."""
    buf = np.zeros(n, np.float32)
    r = lib().heaac_get_table(name.encode(), _np(buf), n)
    if r < 0:
        raise KeyError(name)
    return buf[:r].copy()


def sbr_make_header(sample_rate=48000, start_freq=5, stop_freq=9, xover=0, freq_scale=2,
                    alter_scale=1, noise_bands=2, limiter_bands=2, limiter_gains=2,
                    interpol_freq=1, smoothing_mode=1, amp_res=1):
    """heaac_sbr_make_header(): SBR header -> band tables (host C, no GPU)."""
    h = np.zeros(1, SBR_HDR_DT)
    rc = lib().heaac_sbr_make_header(_np(h), sample_rate, start_freq, stop_freq,
                                     xover, freq_scale, alter_scale, noise_bands, limiter_bands,
                                     limiter_gains, interpol_freq, smoothing_mode, amp_res)
    if rc != 0:
        raise ValueError("invalid SBR header (%d)" % rc)
    return h


def _np(a):
    """Address of a numpy array (or None)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _units(aus):
    """A list of access units (bytes) -> (keep, ptrs, sizes): the buffers (to be held until the call has returned), the
    c_char_p array of their addresses and the c_int array of their sizes."""
    keep = [C.create_string_buffer(bytes(a), len(a)) for a in aus]
    ptrs = (C.c_char_p * len(aus))(*[C.cast(k, C.c_char_p) for k in keep])
    return keep, ptrs, (C.c_int * len(aus))(*[len(a) for a in aus])


def _ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return C.c_void_p(t.data_ptr())


def _hold_ptr(hold, n):
    """The [S][T] hold mask of the *_streams_ex calls: a uint8 tensor of n = S * T elements."""
    import torch
    assert hold.dtype == torch.uint8 and hold.numel() == n, "hold"
    return _ptr(hold)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(a, dtype, shape, name, device):
    """An output tensor of the device parsers: a new one of `shape` when the caller gave none, else the caller's, checked
    (a wrong-length tensor would be a silent device out-of-bounds access; the assertion names the argument)."""
    import torch
    if a is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert a.dtype == dtype and a.numel() == int(np.prod(shape)), name
    return a


def _pcm(pcm, n, channels, length, pcm_format, device):
    """The PCM tensor of a decode call over n frames: float32 [n][channels][length] for PCM_F32, else int16
    [n][length][channels]; a new one when the caller gave none, else the caller's, checked."""
    import torch
    f32 = pcm_format == PCM_F32
    dtype = torch.float32 if f32 else torch.int16
    if pcm is None:
        return torch.empty((n, channels, length) if f32 else (n, length, channels), dtype=dtype, device=device)
    assert pcm.numel() == n * channels * length and pcm.dtype == dtype, "pcm"
    return pcm


def _state_out(state_out, state_in):
    """The state_out tensor of a decode call: a new one like state_in when the caller gave none, else checked."""
    import torch
    if state_out is None:
        return torch.empty_like(state_in)
    assert state_out.dtype == torch.float32 and state_out.numel() == state_in.numel(), "state_out"
    return state_out


def _units_in(streams, au_bytes, au_offset, cc, T=1):
    """The input checks of the device AAC parsers over S streams x T units (one unit per stream: T = 1): returns the
    number of units, S * T."""
    import torch
    assert isinstance(au_offset, torch.Tensor) and au_offset.dtype == torch.int32 and au_offset.numel() >= 1, "au_offset"
    n = au_offset.numel() - 1
    assert n % T == 0, "au_offset: S * T + 1 offsets"
    assert cc in (1, 2), "coeff_channels"
    assert au_bytes.dtype == torch.uint8, "au_bytes"
    assert streams.dtype == torch.uint8 and streams.numel() == n // T * AAC_STREAM_DT.itemsize, "streams"
    return n


def _aac_out(n, cc, coeffs, ics, tools, info, device):
    """The four record arrays of the AAC half for n units: (coeffs, ics, tools, info)."""
    import torch
    return (_out(coeffs, torch.float32, (n, cc, 1024), "coeffs", device),
            _out(ics, torch.uint8, n * cc * ICS_DT.itemsize, "ics", device),
            _out(tools, torch.uint8, n * TOOLS_FRAME_DT.itemsize, "tools", device),
            _out(info, torch.uint8, n * AAC_INFO_DT.itemsize, "info", device))


def to_device(a, device="cuda"):
    """numpy (possibly structured) array -> uint8/float32 torch tensor on the GPU."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names is not None or a.dtype.kind not in "fiu":
        return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)
    return torch.from_numpy(a).to(device)


class Device:
    """HeaacDevice: per-GPU immutable tables (+ workspace)."""

    def __init__(self, max_frames=0):
        import torch
        if not torch.cuda.is_available():
            raise HeaacError("no HIP device visible: the HE-AAC DSP path has no CPU fallback")
        self._h = C.c_void_p()
        _check(lib().heaac_device_create(C.byref(self._h), max_frames), "heaac_device_create")

    def close(self):
        if self._h:
            lib().heaac_device_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def x_bands(self, n):
        """include/heaac_debug.h: the X bands stored per (frame, channel) by the last HE decode call, uint8 [n][2]."""
        buf = np.zeros(2 * n, np.uint8)
        _check(lib().heaac_debug_xbands(self._h, _np(buf), n), "heaac_debug_xbands")
        return buf.reshape(n, 2)

    def x_bands_shares(self, n):
        """include/heaac_debug.h: the share of (frame, channel) X records of the last HE decode call that were
        stored with 32 / 48 / 64 bands, as {"32": .., "48": .., "64": ..}."""
        buf = self.x_bands(n)
        return {str(b): round(float((buf == b).mean()), 4) for b in (32, 48, 64)}

    # -- transforms --
    def imdct_half(self, which, x):
        import torch
        n_half = {0: 1024, 1: 128, 2: 64, 3: 64}[which]
        assert x.dtype == torch.float32 and x.shape[-1] == n_half
        x = x.contiguous()
        out = torch.empty_like(x)
        _check(lib().heaac_imdct_half_batch(self._h, which, _ptr(out), _ptr(x), x.numel() // n_half, _stream()),
               "heaac_imdct_half_batch")
        return out

    # -- AAC-LC --
    @staticmethod
    def _lc_args(channels, coeffs, ics, state_in, S, T, state_out, pcm, pcm_format):
        """The tensors of an LC decode call over S streams x T frames (lc_decode: S = n, T = 1), checked -- a
        wrong-length tensor would be a silent device out-of-bounds access.  Returns (state_out, pcm), allocated where
        the caller gave none."""
        import torch
        n = S * T
        assert state_in.dtype == torch.float32 and state_in.numel() == S * channels * 512, "state_in"
        assert coeffs.dtype == torch.float32 and coeffs.numel() == n * channels * 1024, "coeffs"
        assert ics.numel() * ics.element_size() == n * channels * ICS_DT.itemsize, "ics"
        return _state_out(state_out, state_in), _pcm(pcm, n, channels, 1024, pcm_format, coeffs.device)

    def lc_decode(self, channels, coeffs, ics, state_in, state_out=None, pcm=None, pcm_format=PCM_F32):
        n = coeffs.shape[0]
        state_out, pcm = self._lc_args(channels, coeffs, ics, state_in, n, 1, state_out, pcm, pcm_format)
        _check(lib().heaac_lc_decode_batch(self._h, channels, _ptr(coeffs), _ptr(ics), _ptr(state_in),
                                           _ptr(state_out), _ptr(pcm), pcm_format, n, _stream()),
               "heaac_lc_decode_batch")
        return pcm, state_out

    def lc_decode_streams(self, channels, coeffs, ics, state_in, frames_per_stream, state_out=None, pcm=None,
                          pcm_format=PCM_F32, hold=None):
        """heaac_lc_decode_streams: S streams x T = frames_per_stream consecutive frames each.  The per-frame tensors
        are laid out as for lc_decode with n = S * T (frame t of stream s at s * T + t); state_in / state_out hold ONE
        saved[] record of channels * 512 floats per stream (before frame 0 / after frame T - 1).  hold: None, or a
        uint8 tensor of S * T elements, non-zero = frame held (heaac_lc_decode_streams_ex: skipped, zero PCM, the
        stream's state passes over it).  Returns (pcm, state_out)."""
        T = int(frames_per_stream)
        S = state_in.numel() // (channels * 512)
        state_out, pcm = self._lc_args(channels, coeffs, ics, state_in, S, T, state_out, pcm, pcm_format)
        if hold is None:
            _check(lib().heaac_lc_decode_streams(self._h, channels, _ptr(coeffs), _ptr(ics), _ptr(state_in),
                                                 _ptr(state_out), _ptr(pcm), pcm_format, S, T, _stream()),
                   "heaac_lc_decode_streams")
        else:
            d_hold = _hold_ptr(hold, S * T)
            _check(lib().heaac_lc_decode_streams_ex(self._h, channels, _ptr(coeffs), _ptr(ics), _ptr(state_in),
                                                    _ptr(state_out), _ptr(pcm), pcm_format, S, T, d_hold, _stream()),
                   "heaac_lc_decode_streams_ex")
        return pcm, state_out

    # -- compressed access units -> the records of spectral_tools / lc_decode, on the device --
    def aac_parse(self, cfg, streams, au_bytes, au_offset, coeff_channels=2, coeffs=None, ics=None, tools=None,
                  info=None, status=None):
        """heaac_aac_parse_device: n independent streams, one access unit each; unit i is
        au_bytes[au_offset[i] : au_offset[i + 1]].  streams: uint8 tensor of n AAC_STREAM_DT records (updated in place
        for the units that come back OK), au_bytes: uint8 tensor, au_offset: n + 1 offsets, either a host array (checked
        here against len(au_bytes) and uploaded) or an int32 device tensor the caller vouches for.  Returns the dict
        aac_parse_batch returns, as device tensors (coeffs float32 [n][coeff_channels][1024]; ics, tools, info as
        uint8 records), plus status int32 [n]: PARSE_OK or PARSE_DEFERRED (parse that unit on the host)."""
        import torch
        d_off = au_offset
        if not isinstance(au_offset, torch.Tensor):
            off = np.ascontiguousarray(au_offset, dtype=np.int64).reshape(-1)
            assert off.size >= 1 and off[0] >= 0 and (np.diff(off) >= 0).all() and off[-1] <= au_bytes.numel() and \
                off[-1] < 2 ** 31, "au_offset"
            d_off = torch.from_numpy(off.astype(np.int32)).to(au_bytes.device)
        cc = int(coeff_channels)
        # a wrong-length tensor would be a silent device out-of-bounds access: check them all here
        n = _units_in(streams, au_bytes, d_off, cc)
        dv = au_bytes.device
        coeffs, ics, tools, info = _aac_out(n, cc, coeffs, ics, tools, info, dv)
        status = _out(status, torch.int32, n, "status", dv)
        _check(lib().heaac_aac_parse_device(self._h, C.byref(cfg), _ptr(streams), _ptr(au_bytes), _ptr(d_off), n, cc,
                                            _ptr(coeffs), _ptr(ics), _ptr(tools), _ptr(info), _ptr(status), _stream()),
               "heaac_aac_parse_device")
        return dict(coeffs=coeffs, ics=ics, tools=tools, info=info, status=status)

    # -- the SBR / PS payloads of the same units -> the records of he_decode, on the device --
    def _sbr_parse_args(self, cfg, sst_in, sst_out, rows, n, hdr, sbr, ps, status, dv):
        """rows: the number of HeaacSbrStream records (one per unit, or one per stream); n: the number of units."""
        import torch
        sb = lib().heaac_sbr_stream_bytes()
        assert sst_in.dtype == torch.uint8 and sst_in.numel() == rows * sb, "sst_in"
        sst_out = _out(sst_out, torch.uint8, rows * sb, "sst_out", dv)
        assert hdr.dtype == torch.uint8 and hdr.numel() >= SBR_HDR_DT.itemsize and hdr.numel() % SBR_HDR_DT.itemsize == 0, "hdr"
        sbr = _out(sbr, torch.uint8, n * SBR_FRAME_DT.itemsize, "sbr", dv)
        if ps is not None or (cfg.ps != 0 and cfg.chan_config == 1):
            ps = _out(ps, torch.uint8, n * PS_FRAME_DT.itemsize, "ps", dv)
        status = _out(status, torch.int32, n, "status", dv)
        return sst_out, sbr, ps, status

    def sbr_parse_device(self, cfg, sst_in, au_bytes, au_offset, info, hdr, aac_status=None, sst_out=None, sbr=None,
                         ps=None, status=None):
        """heaac_sbr_parse_device behind aac_parse: sst_in / sst_out: uint8 tensors of n HeaacSbrStream records (the
        two must not overlap; sst_out is allocated when None), au_offset: the int32 device tensor of n + 1 offsets
        aac_parse used, info / aac_status: its `info` and `status`, hdr: uint8 tensor of SBR_HDR_DT records.  ps is
        allocated when cfg.ps != 0 on a mono configuration.  Returns dict(sst=sst_out, sbr, ps, status)."""
        import torch
        assert isinstance(au_offset, torch.Tensor) and au_offset.dtype == torch.int32 and au_offset.numel() >= 1, "au_offset"
        n = au_offset.numel() - 1
        assert au_bytes.dtype == torch.uint8, "au_bytes"
        assert info.dtype == torch.uint8 and info.numel() == n * AAC_INFO_DT.itemsize, "info"
        assert aac_status is None or (aac_status.dtype == torch.int32 and aac_status.numel() == n), "aac_status"
        sst_out, sbr, ps, status = self._sbr_parse_args(cfg, sst_in, sst_out, n, n, hdr, sbr, ps, status, au_bytes.device)
        _check(lib().heaac_sbr_parse_device(self._h, C.byref(cfg), _ptr(sst_in), _ptr(sst_out), _ptr(au_bytes), _ptr(au_offset),
                                            _ptr(info), _ptr(aac_status), n, _ptr(hdr), hdr.numel() // SBR_HDR_DT.itemsize,
                                            _ptr(sbr), _ptr(ps), _ptr(status), _stream()), "heaac_sbr_parse_device")
        return dict(sst=sst_out, sbr=sbr, ps=ps, status=status)

    def heaac_parse_device(self, cfg, streams, sst_in, au_bytes, au_offset, hdr, coeff_channels=2, coeffs=None, ics=None,
                           tools=None, info=None, sst_out=None, sbr=None, ps=None, status=None):
        """heaac_heaac_parse_device: aac_parse and sbr_parse_device as one call (one status per unit, PARSE_OK only
        where both halves took it).  au_offset: an int32 device tensor of n + 1 offsets the caller vouches for.
        Returns the dict of aac_parse plus sst, sbr, ps."""
        cc = int(coeff_channels)
        n = _units_in(streams, au_bytes, au_offset, cc)
        dv = au_bytes.device
        coeffs, ics, tools, info = _aac_out(n, cc, coeffs, ics, tools, info, dv)
        sst_out, sbr, ps, status = self._sbr_parse_args(cfg, sst_in, sst_out, n, n, hdr, sbr, ps, status, dv)
        _check(lib().heaac_heaac_parse_device(self._h, C.byref(cfg), _ptr(streams), _ptr(sst_in), _ptr(sst_out), _ptr(au_bytes),
                                              _ptr(au_offset), n, cc, _ptr(coeffs), _ptr(ics), _ptr(tools),
                                              _ptr(info), _ptr(hdr), hdr.numel() // SBR_HDR_DT.itemsize, _ptr(sbr),
                                              _ptr(ps), _ptr(status), _stream()), "heaac_heaac_parse_device")
        return dict(coeffs=coeffs, ics=ics, tools=tools, info=info, status=status, sst=sst_out, sbr=sbr, ps=ps)

    # -- T consecutive units per stream in one call --
    def _parse_streams_args(self, streams, au_bytes, au_offset, T, cc, coeffs, ics, tools, info, status, taken, hold):
        import torch
        T = int(T)
        assert T >= 1, "frames_per_stream"
        n = _units_in(streams, au_bytes, au_offset, cc, T)
        S = n // T
        dv = au_bytes.device
        coeffs, ics, tools, info = _aac_out(n, cc, coeffs, ics, tools, info, dv)
        coeffs = coeffs.view(n, cc, 1024)
        status = _out(status, torch.int32, n, "status", dv)
        taken = _out(taken, torch.int32, S, "taken", dv)
        hold = _out(hold, torch.uint8, n, "hold", dv)
        return S, T, n, dict(coeffs=coeffs, ics=ics, tools=tools, info=info, status=status, taken=taken, hold=hold)

    def aac_parse_streams(self, cfg, streams, au_bytes, au_offset, frames_per_stream, coeff_channels=2, coeffs=None, ics=None,
                          tools=None, info=None, status=None, taken=None, hold=None):
        """heaac_aac_parse_device_streams: S streams x T = frames_per_stream consecutive units, unit t of stream s at
        index s * T + t.  streams: uint8 tensor of S AAC_STREAM_DT records (updated in place: each stands as after the
        last unit taken), au_offset: int32 device tensor of S * T + 1 offsets the caller vouches for (an empty unit
        stops its stream).  Returns the dict of aac_parse with n = S * T, plus taken int32 [S] (units taken from the
        head of each stream) and hold uint8 [S * T] (the mask of the *_streams_ex decode calls)."""
        cc = int(coeff_channels)
        S, T, n, out = self._parse_streams_args(streams, au_bytes, au_offset, frames_per_stream, cc, coeffs, ics, tools, info,
                                                status, taken, hold)
        _check(lib().heaac_aac_parse_device_streams(self._h, C.byref(cfg), _ptr(streams), _ptr(au_bytes), _ptr(au_offset),
                                                    S, T, cc, _ptr(out["coeffs"]), _ptr(out["ics"]), _ptr(out["tools"]),
                                                    _ptr(out["info"]), _ptr(out["status"]), _ptr(out["taken"]), _ptr(out["hold"]),
                                                    _stream()), "heaac_aac_parse_device_streams")
        return out

    def heaac_parse_device_streams(self, cfg, streams, sst_in, au_bytes, au_offset, hdr, frames_per_stream, coeff_channels=2,
                                   coeffs=None, ics=None, tools=None, info=None, sst_out=None, sbr=None, ps=None, status=None,
                                   taken=None, hold=None):
        """heaac_heaac_parse_device_streams: aac_parse_streams with the SBR / PS payload of every unit behind its AAC
        half.  sst_in / sst_out: uint8 tensors of S HeaacSbrStream records (must not overlap; sst_out is allocated when
        None), hdr: uint8 tensor of SBR_HDR_DT records.  Both states stand as after the last unit taken.  Returns the
        dict of aac_parse_streams plus sst, sbr [S * T], ps [S * T] (None unless cfg.ps != 0 on a mono configuration)."""
        cc = int(coeff_channels)
        S, T, n, out = self._parse_streams_args(streams, au_bytes, au_offset, frames_per_stream, cc, coeffs, ics, tools, info,
                                                status, taken, hold)
        # (the status went through _parse_streams_args)
        sst_out, sbr, ps, _ = self._sbr_parse_args(cfg, sst_in, sst_out, S, n, hdr, sbr, ps, out["status"], au_bytes.device)
        _check(lib().heaac_heaac_parse_device_streams(self._h, C.byref(cfg), _ptr(streams), _ptr(sst_in), _ptr(sst_out),
                                                      _ptr(au_bytes), _ptr(au_offset), S, T, cc,
                                                      _ptr(out["coeffs"]), _ptr(out["ics"]), _ptr(out["tools"]), _ptr(out["info"]),
                                                      _ptr(hdr), hdr.numel() // SBR_HDR_DT.itemsize, _ptr(sbr), _ptr(ps),
                                                      _ptr(out["status"]), _ptr(out["taken"]), _ptr(out["hold"]), _stream()),
               "heaac_heaac_parse_device_streams")
        out.update(sst=sst_out, sbr=sbr, ps=ps)
        return out

    # -- spectral tools before the IMDCT (M/S, intensity stereo, TNS), in place --
    def spectral_tools(self, channels, coeffs, tools, rng=None, pred=None):
        """rng: int32 [n] generator states (updated in place) -> noise substitution runs too.
        pred: float32 [n][channels][672][6] predictor states (in place) -> AAC-Main prediction too."""
        import torch
        n = coeffs.shape[0]
        assert coeffs.dtype == torch.float32 and coeffs.numel() == n * channels * 1024
        assert tools.dtype == torch.uint8 and tools.numel() == n * TOOLS_FRAME_DT.itemsize
        assert rng is None or (rng.dtype == torch.int32 and rng.numel() == n)
        assert pred is None or (pred.dtype == torch.float32 and pred.numel() == n * channels * MAX_PREDICTORS * 6)
        _check(lib().heaac_spectral_tools_batch(self._h, channels, _ptr(coeffs), _ptr(tools), _ptr(rng), _ptr(rng),
                                                _ptr(pred), _ptr(pred), n, _stream()), "heaac_spectral_tools_batch")
        return coeffs

    def spectral_tools_streams(self, channels, coeffs, tools, frames_per_stream, rng=None, pred=None, rng_out=None,
                               pred_out=None, hold=None):
        """heaac_spectral_tools_streams: S streams x T = frames_per_stream consecutive frames each, in place on coeffs.
        coeffs / tools are laid out as for spectral_tools with n = S * T (frame t of stream s at s * T + t).  rng: int32
        [S] generator states, pred: float32 [S][channels][672][6] predictor states -- one record per stream, before
        frame 0; the states after frame T - 1 go to rng_out / pred_out, or in place when those are None.  hold: None, or a uint8
        tensor of S * T elements, non-zero = frame held (heaac_spectral_tools_streams_ex: generator and predictors do
        not move, the frame's coefficient row is unspecified afterwards).  Returns coeffs."""
        import torch
        T = int(frames_per_stream)
        assert T > 0, "frames_per_stream"
        assert coeffs.dtype == torch.float32 and coeffs.numel() % (channels * 1024) == 0, "coeffs"
        n = coeffs.numel() // (channels * 1024)
        # a wrong-length tensor would be a silent device out-of-bounds access: check them all here
        assert n % T == 0, "coeffs: %d frames are not a multiple of frames_per_stream = %d" % (n, T)
        S = n // T
        assert tools.dtype == torch.uint8 and tools.numel() == n * TOOLS_FRAME_DT.itemsize, "tools"
        pred_words = S * channels * MAX_PREDICTORS * 6
        assert rng is None or (rng.dtype == torch.int32 and rng.numel() == S), "rng"
        assert pred is None or (pred.dtype == torch.float32 and pred.numel() == pred_words), "pred"
        assert rng_out is None or (rng is not None and rng_out.dtype == torch.int32 and rng_out.numel() == S), \
            "rng_out"
        assert pred_out is None or (pred is not None and pred_out.dtype == torch.float32 and
                                    pred_out.numel() == pred_words), "pred_out"
        if rng is not None and rng_out is None:
            rng_out = rng
        if pred is not None and pred_out is None:
            pred_out = pred
        state = lambda: (_ptr(rng), _ptr(rng_out), _ptr(pred), _ptr(pred_out))     # (no rng / pred: no rng_out / pred_out)
        if hold is None:
            _check(lib().heaac_spectral_tools_streams(self._h, channels, _ptr(coeffs), _ptr(tools), *state(), S, T, _stream()),
                   "heaac_spectral_tools_streams")
        else:
            d_hold = _hold_ptr(hold, n)
            _check(lib().heaac_spectral_tools_streams_ex(self._h, channels, _ptr(coeffs), _ptr(tools), *state(), S, T, d_hold,
                                                         _stream()), "heaac_spectral_tools_streams_ex")
        return coeffs

    def spectral_tools_ex(self, channels, stages, coeffs, tools, rng=None, pred=None, cce=None, cce_coeffs=None):
        """heaac_spectral_tools_batch_ex: the PRE / POST halves; cce [n][n_cce] records (uint8 tensor) and
        cce_coeffs [n][n_cce][1024] couple into the target in POST."""
        import torch
        n = coeffs.shape[0]
        assert coeffs.dtype == torch.float32 and coeffs.numel() == n * channels * 1024
        assert tools.dtype == torch.uint8 and tools.numel() == n * TOOLS_FRAME_DT.itemsize
        n_cce = 0
        if cce is not None:
            n_cce = cce.numel() // (n * CCE_FRAME_DT.itemsize)
            assert cce.dtype == torch.uint8 and cce.numel() == n * n_cce * CCE_FRAME_DT.itemsize
            assert cce_coeffs.dtype == torch.float32 and cce_coeffs.numel() == n * n_cce * 1024
        _check(lib().heaac_spectral_tools_batch_ex(self._h, channels, stages, _ptr(coeffs), _ptr(tools), _ptr(rng), _ptr(rng),
                                                   _ptr(pred), _ptr(pred),
                                                   _ptr(cce) if n_cce else None, _ptr(cce_coeffs) if n_cce else None,
                                                   n_cce, n, _stream()), "heaac_spectral_tools_batch_ex")
        return coeffs

    # -- HE-AAC --
    def couple_after_imdct(self, channels, pcm, cce, coupling, s16=False):
        """heaac_couple_after_imdct_batch: pcm [n][channels][1024] f32 updated in place; returns the int16
        interleave of the result when s16."""
        import torch
        n = pcm.shape[0]
        assert pcm.dtype == torch.float32 and pcm.numel() == n * channels * 1024, "pcm"
        assert cce.dtype == torch.float32 and cce.numel() == n * 1024, "cce"
        assert coupling.numel() * coupling.element_size() == n * COUPLING_DT.itemsize, "coupling"
        out = torch.empty((n, 1024, channels), dtype=torch.int16, device=pcm.device) if s16 else None
        _check(lib().heaac_couple_after_imdct_batch(self._h, channels, _ptr(pcm), _ptr(cce), _ptr(coupling), _ptr(out), n,
                                                    _stream()), "heaac_couple_after_imdct_batch")
        return out

    def pcm_interleave(self, planes, length, pcm_format=None):
        """heaac_pcm_interleave_batch.  planes: one (tensor, element offset, frame stride in floats) per output channel,
        each tensor float32 on the device holding that channel of all n frames; returns int16 [n][length][channels]."""
        import torch
        fmt = PCM_S16 if pcm_format is None else pcm_format
        ch = len(planes)
        t0, off0, stride0 = planes[0]
        n = (t0.numel() - off0 - length) // stride0 + 1 if stride0 else 1
        refs = (_PlaneRef * ch)()
        for c, (t, off, stride) in enumerate(planes):
            assert t.dtype == torch.float32 and off + (n - 1) * stride + length <= t.numel(), "plane %d" % c
            refs[c].d_base = t.data_ptr() + 4 * off
            refs[c].frame_stride = stride
        out = torch.empty((n, length, ch), dtype=torch.int16, device=t0.device)
        _check(lib().heaac_pcm_interleave_batch(self._h, ch, refs, int(length), int(fmt), _ptr(out), n, _stream()),
               "heaac_pcm_interleave_batch")
        return out

    def he_check(self, cfg, sbr, hdr, ps=None):
        """heaac_he_check_batch on device-resident records (byte tensors as he_decode takes them):
        returns None if every frame is valid, else (first bad frame index, rule name)."""
        n = sbr.numel() // SBR_FRAME_DT.itemsize
        first, rule = C.c_size_t(0), C.c_int(0)
        rc = lib().heaac_he_check_batch(self._h, cfg, sbr.data_ptr(), hdr.data_ptr(), hdr.numel() // SBR_HDR_DT.itemsize,
                                        ps.data_ptr() if ps is not None else None, n, _stream(), C.byref(first), C.byref(rule))
        if rc == 0:
            return None
        if rc != -1:
            _check(rc, "heaac_he_check_batch")
        if first.value == C.c_size_t(-1).value:
            raise HeaacError("heaac_he_check_batch: bad arguments")
        return int(first.value), BAD_RULES[rule.value] if 0 <= rule.value < len(BAD_RULES) else str(rule.value)

    @staticmethod
    def _he_args(cfg, coeffs, ics, sbr, hdr, ps, state_in, S, T, state_out, pcm, pcm_format, downsampled):
        """The tensors of an HE decode call over S streams x T frames (he_decode: S = n, T = 1), checked -- a
        wrong-length tensor would be a silent device out-of-bounds read.  Returns (n_hdr, state_out, pcm), the last two
        allocated where the caller gave none."""
        import torch
        n = S * T
        assert state_in.dtype == torch.float32 and state_in.numel() == S * STATE_WORDS[cfg], "state_in"
        assert coeffs.dtype == torch.float32 and coeffs.numel() == n * CORE_CH[cfg] * 1024, "coeffs"
        assert ics.numel() * ics.element_size() == n * CORE_CH[cfg] * ICS_DT.itemsize, "ics"
        assert sbr.numel() * sbr.element_size() == n * SBR_FRAME_DT.itemsize, "sbr"
        assert hdr.numel() * hdr.element_size() >= SBR_HDR_DT.itemsize and \
            (hdr.numel() * hdr.element_size()) % SBR_HDR_DT.itemsize == 0, "hdr"
        if cfg == CFG_HEV2:
            assert ps is not None and ps.numel() * ps.element_size() == n * PS_FRAME_DT.itemsize, "ps"
        pcm = _pcm(pcm, n, OUT_CH[cfg], 1024 if downsampled else 2048, pcm_format, coeffs.device)
        return hdr.numel() // SBR_HDR_DT.itemsize, _state_out(state_out, state_in), pcm

    def he_decode(self, cfg, coeffs, ics, sbr, hdr, ps, state_in, state_out=None, pcm=None,
                  pcm_format=PCM_F32, downsampled=False):
        """downsampled: HEAAC_HE_DOWNSAMPLED -- output at the core rate, 1024 samples per channel."""
        n = coeffs.shape[0]
        n_hdr, state_out, pcm = self._he_args(cfg, coeffs, ics, sbr, hdr, ps, state_in, n, 1, state_out, pcm, pcm_format,
                                              downsampled)
        _check(lib().heaac_he_decode_batch_ex(self._h, cfg, 1 if downsampled else 0, _ptr(coeffs), _ptr(ics), _ptr(sbr),
                                              _ptr(hdr), n_hdr, _ptr(ps), _ptr(state_in), _ptr(state_out),
                                              _ptr(pcm), pcm_format, n, _stream()),
               "heaac_he_decode_batch")
        return pcm, state_out

    def he_decode_streams(self, cfg, coeffs, ics, sbr, hdr, ps, state_in, frames_per_stream, state_out=None, pcm=None,
                          pcm_format=PCM_F32, downsampled=False, hold=None):
        """heaac_he_decode_streams: S streams x T = frames_per_stream consecutive frames each.  The per-frame tensors
        are laid out as for he_decode with n = S * T (frame t of stream s at s * T + t); state_in / state_out hold ONE
        record per stream (before frame 0 / after frame T - 1).  hold: None, or a uint8 tensor of S * T elements,
        non-zero = frame held (heaac_he_decode_streams_ex).  Returns (pcm, state_out)."""
        T = int(frames_per_stream)
        S = state_in.numel() // STATE_WORDS[cfg]
        n_hdr, state_out, pcm = self._he_args(cfg, coeffs, ics, sbr, hdr, ps, state_in, S, T, state_out, pcm, pcm_format,
                                              downsampled)
        if hold is None:
            _check(lib().heaac_he_decode_streams(self._h, cfg, 1 if downsampled else 0, _ptr(coeffs), _ptr(ics), _ptr(sbr),
                                                 _ptr(hdr), n_hdr, _ptr(ps), _ptr(state_in), _ptr(state_out),
                                                 _ptr(pcm), pcm_format, S, T, _stream()),
                   "heaac_he_decode_streams")
        else:
            d_hold = _hold_ptr(hold, S * T)
            _check(lib().heaac_he_decode_streams_ex(self._h, cfg, 1 if downsampled else 0, _ptr(coeffs), _ptr(ics), _ptr(sbr),
                                                    _ptr(hdr), n_hdr, _ptr(ps), _ptr(state_in), _ptr(state_out),
                                                    _ptr(pcm), pcm_format, S, T, d_hold, _stream()),
                   "heaac_he_decode_streams_ex")
        return pcm, state_out

    def qmf_analysis(self, x, xhist, scale=32768.0):
        import torch
        n = x.shape[0]
        W = torch.empty((n, 32, 32, 2), dtype=torch.float32, device=x.device)
        xh = torch.empty_like(xhist)
        _check(lib().heaac_qmf_analysis_batch(self._h, _ptr(x), _ptr(xhist), _ptr(xh), _ptr(W), scale, n, _stream()),
               "heaac_qmf_analysis_batch")
        return W, xh

    def _qmf_synthesis(self, entry, length, X, v, scale, bias):
        import torch
        n = X.shape[0]
        out = torch.empty((n, length), dtype=torch.float32, device=X.device)
        vo = torch.empty_like(v)
        _check(getattr(lib(), entry)(self._h, _ptr(X), _ptr(v), _ptr(vo), _ptr(out), scale, bias, n, _stream()), entry)
        return out, vo

    def qmf_synthesis(self, X, v, scale=2.0 ** -15, bias=385.0):
        return self._qmf_synthesis("heaac_qmf_synthesis_batch", 2048, X, v, scale, bias)

    def qmf_synthesis_ds(self, X, v, scale=2.0 ** -15, bias=385.0):
        """Downsampled synthesis bank (div = 1): X [n][2][32][64], v [n][576] -> out [n][1024]."""
        return self._qmf_synthesis("heaac_qmf_synthesis_ds_batch", 1024, X, v, scale, bias)


# ---------------------------------------------------------------------------------------------------
# host-side AAC parser (include/heaac_parse.h)
# ---------------------------------------------------------------------------------------------------
class _PlaneRef(C.Structure):
    _fields_ = [("d_base", C.c_void_p), ("frame_stride", C.c_size_t)]


class AacConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("object_type", "sampling_index", "sample_rate", "chan_config", "sbr",
                                       "ext_object_type", "ext_sampling_index", "ext_sample_rate",
                                       "ext_chan_config", "ps")]


class AdtsHeader(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("sample_rate", "samples", "bit_rate", "object_type", "sampling_index",
                                       "chan_config", "crc_absent", "num_aac_frames", "frame_length")]


COUPLING_DT = np.dtype([("gain", "<f4", (2,)), ("on", "u1", (2,)), ("pad", "u1", (2,))])
AAC_STREAM_DT = np.dtype([("window_sequence", "u1", (2,)), ("use_kb_window", "u1", (2,)),
                          ("cce_window_sequence", "u1", (16,)), ("cce_use_kb_window", "u1", (16,)),
                          ("mapped_tag", "u1"), ("oc", "u1"), ("pad", "u1", (2,))])
AAC_INFO_DT = np.dtype([("channels", "<i4"), ("bits_consumed", "<i4"), ("sbr_payload_bit", "<i4"),
                        ("sbr_payload_bytes", "<i4"), ("sbr_crc", "<i4"), ("elem_id", "<i4"), ("n_cce", "<i4"),
                        ("sbr_misplaced", "<i4"), ("refused", "<i4")])
REFUSED_AS_REFERENCE, REFUSED_RUN_TOOLS = 1, 2


def asc_parse(buf):
    """heaac_asc_parse: (AacConfig, bit offset of the specific config)."""
    c = AacConfig()
    r = lib().heaac_asc_parse(C.byref(c), bytes(buf), len(buf))
    if r < 0:
        raise HeaacError("heaac_asc_parse -> %d" % r)
    return c, r


def adts_parse_header(buf):
    h = AdtsHeader()
    r = lib().heaac_adts_parse_header(C.byref(h), bytes(buf), len(buf))
    return h, r


ADTS_PACKET_DT = np.dtype([("offset", "<u8"), ("size", "<u8"), ("kind", "<i4"), ("header_size", "<i4")])
ADTS_FRAME, ADTS_JUNK, ADTS_TRUNCATED, ADTS_TAG = 0, 1, 2, 3


def adts_probe(buf):
    """heaac_adts_probe: the demuxer's probe score of a raw ADTS buffer."""
    return lib().heaac_adts_probe(bytes(buf), len(buf))


def adts_split(buf):
    """heaac_adts_split: (packets [ADTS_PACKET_DT], header of the first frame or None)."""
    buf = bytes(buf)
    n = lib().heaac_adts_split(buf, len(buf), None, 0, None)
    if n < 0:
        raise HeaacError("heaac_adts_split -> %d" % n)
    out = np.zeros(n, ADTS_PACKET_DT)
    h = AdtsHeader()
    m = lib().heaac_adts_split(buf, len(buf), _np(out), n, C.byref(h))
    assert m == n
    return out, (h if (out["kind"] != ADTS_JUNK).any() and ((out["kind"] == ADTS_FRAME) | (out["kind"] == ADTS_TRUNCATED)).any() else None)


PIPELINE_DEVICE_PARSE = 1         # heaac_pipeline.h


class Pipeline:
    """include/heaac_pipeline.h: access units in host memory -> int16 PCM in host memory, ticks overlapped."""

    def __init__(self, aac_cfg, he_cfg, n_streams, threads=0, frames_per_tick=1, device_parse=False):
        """frames_per_tick = T > 1: every tick carries T consecutive access units of each stream
        (heaac_pipeline_create_streams), unit t of stream s at s * T + t.  device_parse: the units are parsed on the GPU
        (heaac_pipeline_create_ex with HEAAC_PIPELINE_DEVICE_PARSE); PCM and statuses are the same."""
        self._h = C.c_void_p()
        self.n, self.ch, self.len = n_streams, OUT_CH[he_cfg], OUT_LEN[he_cfg]
        self.T = int(frames_per_tick)
        if self.len == 2048 and aac_cfg.ext_sample_rate and aac_cfg.ext_sample_rate < 2 * aac_cfg.sample_rate:
            self.len = 1024                                # downsampled SBR: the output at the core rate
        if device_parse:
            _check(lib().heaac_pipeline_create_ex(C.byref(self._h), C.byref(aac_cfg), he_cfg, n_streams, max(self.T, 0), threads,
                                                  PIPELINE_DEVICE_PARSE), "heaac_pipeline_create_ex")
        elif self.T == 1:
            _check(lib().heaac_pipeline_create(C.byref(self._h), C.byref(aac_cfg), he_cfg, n_streams, threads),
                   "heaac_pipeline_create")
        else:
            _check(lib().heaac_pipeline_create_streams(C.byref(self._h), C.byref(aac_cfg), he_cfg, n_streams, max(self.T, 0),
                                                       threads), "heaac_pipeline_create_streams")

    def submit(self, aus, with_status=True):
        """aus: n_streams * frames_per_tick access units (bytes; an empty one where a stream has run out).  Returns the
        parse status per unit (None without a status array)."""
        assert len(aus) == self.n * self.T
        keep, ptrs, sizes = _units(aus)
        status = np.zeros(len(aus), np.int32) if with_status else None
        _check(lib().heaac_pipeline_submit(self._h, ptrs, sizes, _np(status)), "heaac_pipeline_submit")
        return status

    def submit_raw(self, ptrs, sizes):
        _check(lib().heaac_pipeline_submit(self._h, ptrs, sizes, None), "heaac_pipeline_submit")

    def collect(self):
        """PCM of the oldest tick in flight: int16 [n][len][channels], or [n][T][len][channels] with frames_per_tick =
        T > 1 (a view of the pipeline's pinned buffer)."""
        p = C.POINTER(C.c_int16)()
        _check(lib().heaac_pipeline_collect(self._h, C.byref(p)), "heaac_pipeline_collect")
        if self.T == 1:
            return np.ctypeslib.as_array(p, shape=(self.n, self.len, self.ch))
        return np.ctypeslib.as_array(p, shape=(self.n, self.T, self.len, self.ch))

    def timing(self):
        ms = (C.c_float * 4)()
        lib().heaac_pipeline_timing(self._h, ms)
        return dict(parse=ms[0], h2d=ms[1], gpu=ms[2], d2h=ms[3])

    def parse_counts(self):
        """(units the device walk took, units the host parser was handed), cumulative since create"""
        c = (C.c_ulonglong * 2)()
        lib().heaac_pipeline_parse_counts(self._h, c)
        return int(c[0]), int(c[1])

    def close(self):
        if self._h:
            lib().heaac_pipeline_destroy(self._h)
            self._h = C.c_void_p()


class LayoutPipeline:
    """include/heaac_pipeline.h, second half: n streams of one multi-element layout, access units in, int16 PCM out."""

    def __init__(self, aac_cfg, layout, n_streams, threads=0):
        self._h = C.c_void_p()
        self.n, self.ch = n_streams, int(layout[0]["channels"])
        he = aac_cfg.sbr == 1
        self.len = 2048 if he and not (aac_cfg.ext_sample_rate and aac_cfg.ext_sample_rate < 2 * aac_cfg.sample_rate) else 1024
        self._layout = np.ascontiguousarray(layout)
        _check(lib().heaac_layout_pipeline_create(C.byref(self._h), C.byref(aac_cfg), _np(self._layout), n_streams, threads),
               "heaac_layout_pipeline_create")
        self.ch = int(lib().heaac_layout_pipeline_channels(self._h))

    def submit(self, aus):
        assert len(aus) == self.n
        keep, ptrs, sizes = _units(aus)
        status = np.zeros(self.n, np.int32)
        _check(lib().heaac_layout_pipeline_submit(self._h, ptrs, sizes, _np(status)), "heaac_layout_pipeline_submit")
        return status

    def submit_raw(self, ptrs, sizes, status=None):
        """ptrs, sizes: ctypes arrays of n_streams built once by the caller; status: an int32 array of n_streams to
        fill, or None."""
        _check(lib().heaac_layout_pipeline_submit(self._h, ptrs, sizes, _np(status)), "heaac_layout_pipeline_submit")

    def collect(self):
        p = C.POINTER(C.c_int16)()
        _check(lib().heaac_layout_pipeline_collect(self._h, C.byref(p)), "heaac_layout_pipeline_collect")
        return np.ctypeslib.as_array(p, shape=(self.n, self.len, self.ch))

    def close(self):
        if self._h:
            lib().heaac_layout_pipeline_destroy(self._h)
            self._h = C.c_void_p()


class _CceOut(C.Structure):
    _fields_ = [("cce", C.c_void_p), ("coeffs", C.c_void_p), ("ics", C.c_void_p), ("tools", C.c_void_p), ("elem", C.c_void_p)]


def aac_parse_frame_ex(cfg, stream, au, coeff_channels=2, with_cce=True):
    """heaac_aac_parse_frame_ex on one access unit.  `stream`: one AAC_STREAM_DT record (updated in place).
    Returns (status, dict(coeffs [coeff_channels][1024], ics, tools, info, cce [MAX_CCE], cce_coeffs, cce_ics, cce_tools))."""
    au = bytes(au)
    out = dict(coeffs=np.zeros((coeff_channels, 1024), np.float32), ics=np.zeros(2, ICS_DT),
               tools=np.zeros(1, TOOLS_FRAME_DT), info=np.zeros(1, AAC_INFO_DT),
               cce=np.zeros(MAX_CCE, CCE_FRAME_DT), cce_coeffs=np.zeros((MAX_CCE, 1024), np.float32),
               cce_ics=np.zeros(MAX_CCE, ICS_DT), cce_tools=np.zeros(MAX_CCE, TOOLS_FRAME_DT))
    co = _CceOut(out["cce"].ctypes.data, out["cce_coeffs"].ctypes.data, out["cce_ics"].ctypes.data,
                 out["cce_tools"].ctypes.data)
    r = lib().heaac_aac_parse_frame_ex(C.byref(cfg), _np(stream), au, len(au), coeff_channels, _np(out["coeffs"]),
                                       _np(out["ics"]), _np(out["tools"]), C.byref(co) if with_cce else None, _np(out["info"]))
    return r, out


# ---- channel layouts (several output elements per access unit) ----
MAX_ELEMENTS = 16
AAC_ELEM_SLOT_DT = np.dtype([("type", "u1"), ("id", "u1"), ("channels", "u1"), ("first_channel", "u1")])
AAC_LAYOUT_DT = np.dtype([("chan_config", "<i4"), ("n_elements", "<i4"), ("channels", "<i4"), ("tags_mapped", "<i4"),
                          ("channel_layout", "<i8"), ("elem", AAC_ELEM_SLOT_DT, (MAX_ELEMENTS,)),
                          ("slot_of", "i1", (4, 16)), ("tag_map", "i1", (4, 16))])
AAC_ELEM_INFO_DT = np.dtype([("present", "u1"), ("type", "u1"), ("tag", "u1"), ("seq", "u1"), ("sbr_crc", "u1"),
                             ("sbr_misplaced", "u1"), ("pad", "u1", (2,)), ("sbr_payload_bit", "<i4"), ("sbr_payload_bytes", "<i4")])
assert AAC_LAYOUT_DT.itemsize == 216 and AAC_ELEM_INFO_DT.itemsize == 16


def aac_layout_default(chan_config):
    """heaac_aac_layout_default: (status, one AAC_LAYOUT_DT record)."""
    l = np.zeros(1, AAC_LAYOUT_DT)
    return lib().heaac_aac_layout_default(_np(l), int(chan_config)), l


def aac_layout_from_pce(buf, bit_offset):
    """heaac_aac_layout_from_pce: (status, layout, bits used)."""
    l = np.zeros(1, AAC_LAYOUT_DT)
    used = C.c_int(0)
    buf = bytes(buf)
    r = lib().heaac_aac_layout_from_pce(_np(l), buf, len(buf), int(bit_offset), C.byref(used))
    return r, l, used.value


def aac_layout_from_au(au):
    """heaac_aac_layout_from_au: (status, layout)."""
    l = np.zeros(1, AAC_LAYOUT_DT)
    au = bytes(au)
    return lib().heaac_aac_layout_from_au(_np(l), au, len(au)), l


def asc_layout(buf):
    """heaac_asc_layout: (status, AacConfig, layout)."""
    c = AacConfig()
    l = np.zeros(1, AAC_LAYOUT_DT)
    buf = bytes(buf)
    return lib().heaac_asc_layout(C.byref(c), _np(l), buf, len(buf)), c, l


def aac_parse_frame_layout(cfg, layout, streams, au, with_cce=False):
    """heaac_aac_parse_frame_layout (with_cce: heaac_aac_parse_frame_layout_ex) on one access unit.  layout: one
    AAC_LAYOUT_DT record (its tag map is updated), streams: AAC_STREAM_DT [n_elements] (updated).  Returns (status,
    dict(coeffs [ne][2][1024], ics [ne][2], tools [ne], elem [ne], info; with_cce: cce [ne][MAX_CCE], cce_coeffs
    [MAX_CCE][1024], cce_ics [MAX_CCE], cce_tools [MAX_CCE], cce_elem [MAX_CCE] (not handed over when
    with_cce == "no_sbr")))."""
    au = bytes(au)
    ne = int(layout[0]["n_elements"])
    assert streams.dtype == AAC_STREAM_DT and streams.shape[0] >= ne
    out = dict(coeffs=np.zeros((ne, 2, 1024), np.float32), ics=np.zeros((ne, 2), ICS_DT), tools=np.zeros(ne, TOOLS_FRAME_DT),
               elem=np.zeros(ne, AAC_ELEM_INFO_DT), info=np.zeros(1, AAC_INFO_DT))
    args = (C.byref(cfg), _np(layout), _np(streams), au, len(au), _np(out["coeffs"]), _np(out["ics"]), _np(out["tools"]),
            _np(out["elem"]))
    if not with_cce:
        return lib().heaac_aac_parse_frame_layout(*args, _np(out["info"])), out
    out.update(cce=np.zeros((ne, MAX_CCE), CCE_FRAME_DT), cce_coeffs=np.zeros((MAX_CCE, 1024), np.float32),
               cce_ics=np.zeros(MAX_CCE, ICS_DT), cce_tools=np.zeros(MAX_CCE, TOOLS_FRAME_DT),
               cce_elem=np.zeros(MAX_CCE, AAC_ELEM_INFO_DT))
    co = _CceOut(out["cce"].ctypes.data, out["cce_coeffs"].ctypes.data, out["cce_ics"].ctypes.data,
                 out["cce_tools"].ctypes.data, out["cce_elem"].ctypes.data if with_cce != "no_sbr" else None)
    return lib().heaac_aac_parse_frame_layout_ex(*args, C.byref(co), _np(out["info"])), out


def aac_parse_batch(cfg, streams, aus, threads=0):
    """heaac_aac_parse_batch over a list of access units (bytes), one per stream.  `streams`: AAC_STREAM_DT
    array updated in place.  Returns dict(coeffs [n][2][1024], ics [n][2], tools [n], info [n], status [n])."""
    n = len(aus)
    keep, ptrs, sizes = _units(aus)
    out = dict(coeffs=np.zeros((n, 2, 1024), np.float32), ics=np.zeros((n, 2), ICS_DT),
               tools=np.zeros(n, TOOLS_FRAME_DT), info=np.zeros(n, AAC_INFO_DT), status=np.zeros(n, np.int32))
    assert streams.dtype == AAC_STREAM_DT and streams.shape == (n,)
    out["failed"] = lib().heaac_aac_parse_batch(C.byref(cfg), _np(streams), ptrs, sizes, n, _np(out["coeffs"]), _np(out["ics"]),
                                                _np(out["tools"]), _np(out["info"]), _np(out["status"]), threads)
    return out


PARSE_OK, PARSE_DEFERRED = 0, 1
PARSE_WHY_PULSE, PARSE_WHY_ELEMENT, PARSE_WHY_REFUSED = 1, 2, 4


def pack_units(aus):
    """A list of access units (bytes) -> (uint8 array of all of them back to back, int64 offsets [n + 1])."""
    off = np.zeros(len(aus) + 1, np.int64)
    np.cumsum([len(a) for a in aus], out=off[1:])
    return np.frombuffer(b"".join(bytes(a) for a in aus), np.uint8).copy(), off


def _packed(aus):
    """pack_units for the host walks of the device parsers: (bytes, uint32 offsets), the bytes with one more behind them
    (a pointer even when every unit is empty)."""
    buf, off = pack_units(aus)
    return np.concatenate([buf, np.zeros(1, np.uint8)]), off.astype(np.uint32)


def aac_parse_core(cfg, streams, aus, coeff_channels=2, out=None):
    """heaac_debug_aac_parse_core (include/heaac_debug.h): the walk of heaac_aac_parse_device on the host, over a
    list of access units, one per stream.  `streams`: AAC_STREAM_DT array, updated in place for the units that come
    back PARSE_OK.  Returns the dict of aac_parse_batch (coeffs [n][coeff_channels][1024], ics [n][coeff_channels])
    plus why [n]: 0, or the PARSE_WHY_* reason a unit was deferred for.  `out`: a dict of pre-filled arrays to write into."""
    n = len(aus)
    keep, off = _packed(aus)
    if out is None:
        out = dict(coeffs=np.zeros((n, coeff_channels, 1024), np.float32), ics=np.zeros((n, coeff_channels), ICS_DT),
                   tools=np.zeros(n, TOOLS_FRAME_DT), info=np.zeros(n, AAC_INFO_DT))
    out["status"] = np.zeros(n, np.int32)
    out["why"] = np.zeros(n, np.int32)
    assert streams.dtype == AAC_STREAM_DT and streams.shape == (n,)
    rc = lib().heaac_debug_aac_parse_core(C.byref(cfg), _np(streams), _np(keep), _np(off), n, coeff_channels,
                                          _np(out["coeffs"]), _np(out["ics"]), _np(out["tools"]), _np(out["info"]),
                                          _np(out["status"]), _np(out["why"]))
    _check(rc, "heaac_debug_aac_parse_core")
    return out


SBR_WHY_HEADER, SBR_WHY_HDR_INDEX, SBR_WHY_MISPLACED, SBR_WHY_REFUSED, SBR_WHY_AAC = 1, 2, 4, 8, 16


def sbr_parse_core(cfg, sst_in, aus, info, hdr, aac_status=None, with_ps=True, out=None):
    """heaac_debug_sbr_parse_core (include/heaac_debug.h): the walk of heaac_sbr_parse_device on the host.  sst_in:
    sbr_streams(n) rows (left alone), aus: the access units, info: AAC_INFO_DT [n] as the AAC parser left it, hdr:
    SBR_HDR_DT records, aac_status: int32 [n] or None.  Returns dict(sst [n][bytes], sbr [n], ps [n] or None, status
    [n], why [n]: 0 or the SBR_WHY_* reason).  `out`: a dict of pre-filled sst / sbr / ps arrays to write into."""
    n = len(aus)
    keep, off = _packed(aus)
    sst_in = np.ascontiguousarray(sst_in)
    info = np.ascontiguousarray(info, dtype=AAC_INFO_DT)
    hdr = np.ascontiguousarray(hdr, dtype=SBR_HDR_DT).reshape(-1)
    assert sst_in.dtype == np.uint8 and sst_in.shape[0] == n and info.shape == (n,)
    if out is None:
        out = dict(sst=np.zeros_like(sst_in), sbr=np.zeros(n, SBR_FRAME_DT), ps=np.zeros(n, PS_FRAME_DT) if with_ps else None)
    out["status"] = np.zeros(n, np.int32)
    out["why"] = np.zeros(n, np.int32)
    if aac_status is not None:
        aac_status = np.ascontiguousarray(aac_status, dtype=np.int32)
    rc = lib().heaac_debug_sbr_parse_core(C.byref(cfg), _np(sst_in), _np(out["sst"]), _np(keep), _np(off), _np(info),
                                          _np(aac_status), n, _np(hdr), hdr.shape[0], _np(out["sbr"]), _np(out.get("ps")),
                                          _np(out["status"]), _np(out["why"]))
    _check(rc, "heaac_debug_sbr_parse_core")
    return out


PARSE_WHY_SBR, PARSE_WHY_STOPPED = 256, 1 << 20


def parse_core_streams(cfg, streams, aus, frames_per_stream, coeff_channels=2, sst_in=None, hdr=None, with_ps=True, out=None):
    """heaac_debug_aac_parse_core_streams, or with sst_in (sbr_streams(S) rows, left alone) and hdr (SBR_HDR_DT
    records) heaac_debug_heaac_parse_core_streams (include/heaac_debug.h): the chains of the device streams parsers on
    the host.  aus: S * T access units, unit t of stream s at s * T + t (b"" stops its stream); streams: AAC_STREAM_DT
    [S], updated in place.  Returns dict(coeffs, ics, tools, info, status [S * T], taken [S], hold [S * T], why [S * T])
    plus sst [S][bytes], sbr, ps for HE.  `out`: a dict of pre-filled arrays to write into."""
    T = int(frames_per_stream)
    n = len(aus)
    S = n // T
    assert S * T == n and streams.dtype == AAC_STREAM_DT and streams.shape == (S,)
    he = sst_in is not None
    keep, off = _packed(aus)
    out = dict(out) if out is not None else {}
    out.setdefault("coeffs", np.zeros((n, coeff_channels, 1024), np.float32))
    out.setdefault("ics", np.zeros((n, coeff_channels), ICS_DT))
    out.setdefault("tools", np.zeros(n, TOOLS_FRAME_DT))
    out.setdefault("info", np.zeros(n, AAC_INFO_DT))
    out.setdefault("status", np.zeros(n, np.int32))
    out.setdefault("taken", np.zeros(S, np.uint32))
    out.setdefault("hold", np.zeros(n, np.uint8))
    out.setdefault("why", np.zeros(n, np.int32))
    aac = [_np(out[k]) for k in ("coeffs", "ics", "tools", "info")]
    tail = [_np(out[k]) for k in ("status", "taken", "hold", "why")]
    if not he:
        rc = lib().heaac_debug_aac_parse_core_streams(C.byref(cfg), _np(streams), _np(keep), _np(off), S, T, coeff_channels,
                                                      *aac, *tail)
        _check(rc, "heaac_debug_aac_parse_core_streams")
        return out
    sst_in = np.ascontiguousarray(sst_in)
    hdr = np.ascontiguousarray(hdr, dtype=SBR_HDR_DT).reshape(-1)
    assert sst_in.dtype == np.uint8 and sst_in.shape[0] == S
    out.setdefault("sst", np.zeros_like(sst_in))
    out.setdefault("sbr", np.zeros(n, SBR_FRAME_DT))
    out.setdefault("ps", np.zeros(n, PS_FRAME_DT) if with_ps else None)
    rc = lib().heaac_debug_heaac_parse_core_streams(C.byref(cfg), _np(streams), _np(sst_in), _np(out["sst"]), _np(keep), _np(off),
                                                    S, T, coeff_channels, *aac, _np(hdr), hdr.shape[0], _np(out["sbr"]),
                                                    _np(out["ps"]), *tail)
    _check(rc, "heaac_debug_heaac_parse_core_streams")
    return out


# ---------------------------------------------------------------------------------------------
# heaac_parse.h, second slice: SBR / PS payloads
# ---------------------------------------------------------------------------------------------
SBR_PARSE_INFO_DT = np.dtype([("sbr_bits", "<i4"), ("header", "<i4"), ("ps_present", "<i4"), ("ps_status", "<i4")])
PARSE_NO_SBR = 1


class SbrHeaderTable:
    """heaac_sbr_table_*: the batch's table of derived SBR headers (entry 0 = the null header)."""

    def __init__(self, capacity=256):
        self._h = lib().heaac_sbr_table_create(capacity)
        if not self._h:
            raise HeaacError("heaac_sbr_table_create failed")

    def __len__(self):
        return lib().heaac_sbr_table_count(self._h)

    def headers(self):
        """Copy of the entries so far as an SBR_HDR_DT array (what he_decode takes as `hdr`)."""
        n = len(self)
        addr = lib().heaac_sbr_table_data(self._h)
        buf = (C.c_uint8 * (n * SBR_HDR_DT.itemsize)).from_address(addr)
        return np.frombuffer(bytes(buf), dtype=SBR_HDR_DT).copy()

    def close(self):
        if self._h:
            lib().heaac_sbr_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sbr_streams(n):
    """n fresh HeaacSbrStream records (opaque bytes, heaac_sbr_stream_init)."""
    st = np.zeros((n, lib().heaac_sbr_stream_bytes()), np.uint8)
    lib().heaac_sbr_stream_init(_np(st), n)
    return st


def sbr_parse_payload(stream, table, sample_rate, payload, channels, allow_ps, crc=False, bit=0, cnt=None, misplaced=False):
    """heaac_sbr_parse_payload on ONE stream record (a row of sbr_streams()).  `payload`: the bytes that
    follow the 4-bit extension type when bit = 0 (tests), or a whole access unit with `bit` set.
    Returns (status, sbr record, ps record, info)."""
    assert stream.dtype == np.uint8 and stream.flags["C_CONTIGUOUS"]
    payload = bytes(payload)
    sbr = np.zeros(1, SBR_FRAME_DT)
    ps = np.zeros(1, PS_FRAME_DT)
    info = np.zeros(1, SBR_PARSE_INFO_DT)
    r = lib().heaac_sbr_parse_payload(_np(stream), table._h, sample_rate, payload, len(payload), bit,
                                      len(payload) if cnt is None else cnt, bool(crc), channels,
                                      int(bool(allow_ps)) | (2 if misplaced else 0), _np(sbr), _np(ps), _np(info))
    return r, sbr, ps, info[0]


def sbr_no_payload(stream, channels):
    """heaac_sbr_no_payload: the record of an access unit without an SBR payload for ONE stream record."""
    sbr = np.zeros(1, SBR_FRAME_DT)
    lib().heaac_sbr_no_payload(_np(stream), channels, _np(sbr), None)
    return sbr


def heaac_parse_batch(cfg, streams, sbr_st, table, aus, threads=0, with_ps=False):
    """heaac_heaac_parse_batch: whole HE-AAC access units, one per stream.  streams: AAC_STREAM_DT [n],
    sbr_st: sbr_streams(n); both updated in place.  Returns the dict of aac_parse_batch plus sbr [n], ps [n]."""
    n = len(aus)
    keep, ptrs, sizes = _units(aus)
    out = dict(coeffs=np.zeros((n, 2, 1024), np.float32), ics=np.zeros((n, 2), ICS_DT),
               tools=np.zeros(n, TOOLS_FRAME_DT), info=np.zeros(n, AAC_INFO_DT), status=np.zeros(n, np.int32),
               sbr=np.zeros(n, SBR_FRAME_DT), ps=np.zeros(n, PS_FRAME_DT))
    assert streams.dtype == AAC_STREAM_DT and streams.shape == (n,) and sbr_st.shape[0] == n
    out["failed"] = lib().heaac_heaac_parse_batch(
        C.byref(cfg), _np(streams), _np(sbr_st), table._h, ptrs, sizes, n, _np(out["coeffs"]), _np(out["ics"]),
        _np(out["tools"]), _np(out["sbr"]), _np(out["ps"]) if with_ps else None, _np(out["info"]), _np(out["status"]), threads)
    return out

"""The structural campaign reaches the structure (CPU, oracle only): every profile of tests/edge_grids.py, on exactly
the frames tests/test_grids_gpu.py runs, passes the record validator, runs through the oracle with finite PCM and
state, and holds the classes of grid it is for -- counted, against floors the generators are built to meet -- so that
the GPU parity test on these inputs says something about those classes.  One test records the baseline: the plain
synth with every event on reaches none of them.

test_oracle_defined_on_free_grids runs the oracle on the `free` and `ps_free` records as a stand-alone program under
AddressSanitizer + UBSan (tests/c/oracle_grids.c).  It found one thing: sbr_hf_assemble copies the four smoothing
history rows from 2 t_env_num_env_old to 2 t_env[0] with memcpy (aacsbr.c:1638-1639), and a record may place the two
within one border of each other (a parsed stream never does: the old border is 16..19, or 0 with reset set), where
that copy is undefined.  The value is DEFINED rather than the validator tightened, as DESIGN s1 does for the other
stale reads: the rows move as by memmove (oracle/or_sbr.c hf_assemble), which is what the kernels' ring seeding
(k_hf.h) computes."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import edge_grids as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "c", "_build")
EXE = os.path.join(BUILD, "oracle_grids")


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


def _frames(pkg, profile, cfgname, ps_mode):
    synth = _synth()
    hdr = G.headers(pkg, synth, profile)
    cfg = getattr(pkg, cfgname)
    return cfg, hdr, G.he_frames(pkg, synth, cfg, profile, G.STREAMS, G.STEPS, G.SEED, hdr, ps_mode=ps_mode)


def _valid(pkg, cfg, hdr, frames):
    for t, fr in enumerate(frames):
        for s in range(fr["sbr"].shape[0]):
            r = pkg.validate_frame(cfg, fr["sbr"][s], hdr, fr["ps"][s] if fr["ps"] is not None else None)
            assert r == "NONE", "frame %d stream %d: %s" % (t, s, r)


def _oracle_finite(pkg, oracle, cfg, hdr, frames, ds):
    n = frames[0]["coeffs"].shape[0]
    state = np.zeros((n, pkg.STATE_WORDS[cfg]), np.float32)
    for t, fr in enumerate(frames):
        pcm, state = oracle.he_decode_batch(cfg, fr["coeffs"], fr["ics"], fr["sbr"], hdr, fr["ps"], state,
                                            oracle.PCM_F32, downsampled=ds)
        assert np.isfinite(pcm).all() and np.isfinite(state).all(), t


def _at_least(c, floors):
    low = {k: (c[k], v) for k, v in floors.items() if c[k] < v}
    assert not low, "below the floor (count, floor): %s" % low


# Floors: fixed counts the generators are built to meet with STREAMS x STEPS = 24 x 8 = 192 frames per run (conditions,
# not measurements).  A categorical choice that cycles over k values with stream + frame comes up 192 / k times on the
# first channel alone; the floors sit below that.
def _sbr_floors(profile, c):
    if profile == "five_env":
        assert c["L", 5] == c["grids"]                         # every started frame
        # 7 pointer values in turn (27 each); the widest-limiter header is the 8th of 8: 3 streams x 8 frames
        _at_least(c, dict([(("L", 5), 190), ("L5_widest", 20), ("steps_6_8", 100), ("t_q1_no_border", 10)] +
                          [(("pointer", p), 20) for p in range(7)]))
    elif profile == "narrow":
        # 8 grids in turn, 24 frames each: 4 of them open with a one-slot envelope, 3 close with one, 3 hold four
        # one-slot envelopes in a row (three adjacent pairs each)
        _at_least(c, dict(first_one_slot=80, last_one_slot=60, one_slot_pairs=80, longest=20, shortest=20,
                          t_q1_no_border=10))
    elif profile == "seams":
        assert c["gap", 1] + c["gap", 2] + c["gap", 3] + c["overlap", 1] + c["overlap", 2] + c["overlap", 3] == \
            c["grids"]                                         # no frame starts where the last one ended
        # six seams in turn, 32 each but for the streams' first frames (no overlap with nothing)
        _at_least(c, dict([((k, g), 20) for k in ("gap", "overlap") for g in (1, 2, 3)] +
                          [("seam_reset", 20), ("seam_no_reset", 100), ("seam_smoothing", 40), ("seam_plain", 40)]))
    elif profile == "free":
        # L in turn (38 each); t_q[1] uniform over 20 slots against at most 6 borders; the old border uniform over 20
        _at_least(c, dict([(("L", L), 30) for L in range(1, 6)] + [("t_q1_no_border", 60), ("t_old_below_16", 100)]))
        seen = {k[1:] for k in c if isinstance(k, tuple) and k[0] == "e_a"}
        assert seen >= {(a, b) for a in (-1, 0) for b in range(-1, 6)}     # every (e_a[0], e_a[1]) there is


def _ps_floors(profile, c):
    if profile == "aligned_uneven":
        assert c["aligned_uneven"] == c["frames"]
        _at_least(c, {("borders", tuple(b)): 30 for b in G.ALIGNED_UNEVEN})          # 5 sets in turn, 38 each
    elif profile == "ps_narrow":
        _at_least(c, {("E", 5): 60, "first_one_slot": 100, "last_one_slot": 100})    # 8 grids in turn, 24 each
    elif profile == "ps_free":
        _at_least(c, dict([(("E", E), 30) for E in range(1, 6)] + [(("num_env_old", k), 10) for k in range(6)]))


@pytest.mark.parametrize("profile,cfgname,ps_mode,ds", G.cases())
def test_profile_is_valid_finite_and_not_vacuous(pkg, oracle, profile, cfgname, ps_mode, ds):
    cfg, hdr, frames = _frames(pkg, profile, cfgname, ps_mode)
    _valid(pkg, cfg, hdr, frames)
    _oracle_finite(pkg, oracle, cfg, hdr, frames, ds)
    if profile in G.SBR_PROFILES:
        widest = len(hdr) - 1 if profile == "five_env" else None
        _sbr_floors(profile, G.sbr_counts(frames, hdr, 2 if cfg == pkg.CFG_HEV1 else 1, widest))
    else:
        c = G.ps_counts(frames)
        _ps_floors(profile, c)
        if profile == "ps_free" and ps_mode == "mix":
            _at_least(c, {"layout_switch": 40, ("ipdopd", 0): 40, ("ipdopd", 1): 40})


def test_widest_limiter_header(pkg):
    """edge_grids.WIDEST_LIMITER has m = 48 and the largest n_lim any header with m = 48 has: a search over every
    sampling rate and header field that shapes the band tables (the noise bands shape neither m nor the limiter
    table; limiter_bands = 3 is the densest setting, the others are tried wherever m = 48)"""
    h = pkg.sbr_make_header(**G.WIDEST_LIMITER)[0]
    assert int(h["m"]) == 48 and int(h["n_lim"]) == G.WIDEST_N_LIM
    best = 0
    for rate in (16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000):
        for start in range(16):
            for stop in range(16):
                for xover in range(8):
                    for scale in range(4):
                        for alter in range(2):
                            for bands in (3, 2, 1):
                                try:
                                    z = pkg.sbr_make_header(sample_rate=rate, start_freq=start, stop_freq=stop,
                                                            xover=xover, freq_scale=scale, alter_scale=alter,
                                                            limiter_bands=bands)[0]
                                except ValueError:
                                    break
                                if int(z["m"]) != 48:
                                    break
                                best = max(best, int(z["n_lim"]))
    assert best == G.WIDEST_N_LIM, best


@pytest.mark.parametrize("channels", [1, 2])
def test_window_chains_visit_every_combination(pkg, channels):
    """all 16 (window_sequence, previous) x 4 (shape, previous shape) combinations per channel, in true chains"""
    synth = _synth()
    hdr = synth.default_headers(pkg, extra=True)
    runs = [[ics for _, ics in G.lc_window_frames(pkg, synth, channels, G.SEED)]]
    cfg = pkg.CFG_HEV1 if channels == 2 else pkg.CFG_HEV2
    runs.append([fr["ics"] for fr in G.he_window_frames(pkg, synth, cfg, G.SEED, hdr)])
    for ics in runs:
        for c in range(channels):
            assert len(G.window_combinations(ics, c)) == 64
            for t in range(1, len(ics)):
                assert np.array_equal(ics[t]["window_sequence"][:, c, 1], ics[t - 1]["window_sequence"][:, c, 0])
                assert np.array_equal(ics[t]["use_kb_window"][:, c, 1], ics[t - 1]["use_kb_window"][:, c, 0])
        if channels == 2:
            assert not np.array_equal(ics[0]["window_sequence"][:, 0], ics[0]["window_sequence"][:, 1])


@pytest.mark.parametrize("cfgname", ["CFG_HEV1", "CFG_HEV2"])
def test_window_chains_stay_finite_in_the_he_core(pkg, oracle, cfgname):
    synth = _synth()
    hdr = synth.default_headers(pkg, extra=True)
    cfg = getattr(pkg, cfgname)
    frames = G.he_window_frames(pkg, synth, cfg, G.SEED, hdr)
    _valid(pkg, cfg, hdr, frames)
    _oracle_finite(pkg, oracle, cfg, hdr, frames, False)


def test_plain_synth_reaches_none_of_these_classes(pkg):
    """The baseline the campaign exists for: synth.he_stream with every event on, 200 streams x 12 frames, HE-AACv1
    and v2, never makes five envelopes, never starts a frame off the last one's end, never sends an uneven PS grid
    with every border at 8k - 1, and walks 7 of the 16 window-sequence pairs.  A change to the synth that closes part
    of the gap fails here and is noticed."""
    synth = _synth()
    hdr = synth.default_headers(pkg, extra=True, null=True)
    for cfg, ncore in ((pkg.CFG_HEV1, 2), (pkg.CFG_HEV2, 1)):
        rng = np.random.default_rng(7)
        n = 200
        frames = list(synth.he_stream(rng, cfg, n, 12, hdr, hdr_choice=np.arange(n) % (len(hdr) - 1), coupling=0.5,
                                      events=dict(lead_in=3, p_switch=0.04, p_drop=0.03, p_ps_off=0.03)))
        c = G.sbr_counts(frames, hdr, ncore)
        assert c["grids"] > 1500
        assert c["L", 5] == 0 and {k[1] for k in c if isinstance(k, tuple) and k[0] == "L"} == {1, 2, 3, 4}
        assert not [k for k in c if isinstance(k, tuple) and k[0] in ("gap", "overlap")]
        if cfg == pkg.CFG_HEV2:
            p = G.ps_counts(frames)
            assert p["frames"] > 1500 and p["aligned_uneven"] == 0 and p["E", 5] == 0
        pairs = set()
        for ch in range(ncore):
            pairs |= {k[:2] for k in G.window_combinations([fr["ics"] for fr in frames], ch)}
        assert len(pairs) == 7, sorted(pairs)


def _dump(f, cfg, flags, fmt, hdr, frames):
    n = frames[0]["coeffs"].shape[0]
    f.write(struct.pack("<6i", cfg, flags, fmt, n, len(frames), len(hdr)))
    f.write(np.ascontiguousarray(hdr).tobytes())
    for fr in frames:
        for k in ("coeffs", "ics", "sbr", "ps"):
            if fr[k] is not None:
                f.write(np.ascontiguousarray(fr[k]).tobytes())


def test_oracle_defined_on_free_grids(pkg, oracle):
    """the oracle on the `free` and `ps_free` records, every configuration, both banks and PCM formats, as a
    stand-alone program under AddressSanitizer + UBSan (see the module's docstring for what it found)"""
    os.makedirs(BUILD, exist_ok=True)
    odir = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(ROOT, "tests", "c", "oracle_grids.c")] + sorted(
        os.path.join(odir, f) for f in os.listdir(odir) if f.endswith(".c"))
    deps = srcs + [os.path.join(odir, "oracle.h"), os.path.join(ROOT, "include", "heaac_dsp.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-math-errno", "-ffp-contract=off",
                               "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", odir] + srcs +
                              ["-o", EXE, "-lm"])
    records = os.path.join(BUILD, "grids.bin")
    runs = 0
    with open(records, "wb") as f:
        for profile, cfgname, ps_mode, _ in G.cases():
            if profile not in ("free", "ps_free"):
                continue
            cfg, hdr, frames = _frames(pkg, profile, cfgname, ps_mode)
            _dump(f, cfg, 0, oracle.PCM_F32, hdr, frames)
            _dump(f, cfg, 1, oracle.PCM_S16, hdr, frames)          # HEAAC_HE_DOWNSAMPLED
            runs += 2
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE, records], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=env)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    assert "runs %d, frames %d" % (runs, runs * G.STREAMS * G.STEPS) in p.stdout, p.stdout[-500:]

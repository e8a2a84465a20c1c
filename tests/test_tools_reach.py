"""The spectral tools' campaign reaches what it is for (CPU, oracle only): every profile of tests/edge_tools.py, on
exactly the records tests/test_tools_grid_gpu.py runs, stays inside what a band table gives, runs through the oracle
with finite coefficients, generator and predictors, and holds the classes of record it was built for -- counted,
against floors the generators are built to meet -- so that bit identity on the GPU says something about those
classes.  One test records the baseline: synth.tools_frames, which every other tools test draws from, reaches none of
them.

test_oracle_defined_on_tools_records runs the oracle on all four profiles, mono and stereo, as a stand-alone program
under AddressSanitizer + UBSan (tests/c/oracle_tools.c).  It found nothing: on records a band table gives, every
read of oracle/or_tools.c is inside its record, so nothing had to be defined as DESIGN s1 does for the stale reads of
the SBR records."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import edge_tools as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "c", "_build")
EXE = os.path.join(BUILD, "oracle_tools")


def _at_least(c, floors):
    low = {k: (c[k], v) for k, v in floors.items() if c[k] < v}
    assert not low, "below the floor (count, floor): %s" % low


# Floors: conditions the generators are built to meet with STREAMS x STEPS = 26 x 8 = 208 frames per run (bands:
# 400 x 2), not measurements.  A choice that cycles over k values comes up 208 / k times on channel 0 alone; the floors
# sit below that, and are asked of the mono run (channel 0 alone) as of the stereo one.
def _floors_tables(c, channels):
    # stream s has sampling index s % 13: two streams an index, long and short alternating, so 8 frames of each
    # window length per index on channel 0; the (at most 7) max_sfb choices take the 8 turns
    assert E.keys(c, "si") == {(si, nw) for si in range(E.NUM_SI) for nw in (1, 8)}
    assert {k[1] for k in E.keys(c, "num_swb") if k[0] == 1} == {40, 41, 43, 47, 49, 51}
    assert {k[1] for k in E.keys(c, "num_swb") if k[0] == 8} == {12, 14, 15}
    for si in range(E.NUM_SI):
        for eight in (False, True):
            for m in E.max_sfb_choices(si, eight):
                assert c["max_sfb_at", 8 if eight else 1, E.first_si(si, eight), m] >= 1, (si, eight, m)
    _at_least(c, {("max_sfb", 0): 26, ("max_sfb", 1): 26})         # 26 (index, window length) pairs, once each
    if channels == 2:
        # common_window 0 on a third of the frames: the other window length and another max_sfb on channel 1
        _at_least(c, dict(windows_differ=60, max_sfb_differ=40))


def _floors_tns_orders(c, channels):
    for nw in (1, 8):                                              # 21 orders x 2 directions, on filters that run
        assert {k[1:] for k in E.keys(c, "tns") if k[0] == nw} == {(o, d) for o in range(21) for d in (0, 1)}, nw
    # six length patterns in turn, 34 frames each, half of them long; 20 of 26 streams walk the orders
    _at_least(c, dict(tiles=10, clamped=10, empty_after_clamp=10, empty_length_0=10, empty_above=10, straddle=30,
                      order_gt_size=10, order20_on_4_lines=5))


def _floors_bands(c, channels):
    for nswb in (12, 14, 15):                                      # 384 streams: grouping s % 128 on class s // 128
        assert {k[1] for k in E.keys(c, "grouping") if k[0] == nswb} == set(range(128)), nswb
    # eight specials in turn over 416 frames, 52 each
    _at_least(c, {("bands", 120): 200, ("noise_bands", 120): 40, "second_round_full": 80, "all_noise": 80,
                  ("noise_width", 96): 40, ("noise_width", 4): 40, "frame_max_sfb_0": 40})
    if channels == 2:
        _at_least(c, {("all_intensity", 0): 10, ("all_intensity", 1): 10, ("all_intensity", 2): 10,
                      "ms_skips_noise": 52 * 60})                  # 80 of a frame's 120 bands have noise on one side


def _floors_prediction(c, channels):
    # reset group (8 s + k) % 31 on channel 0: every value six or seven times, short frames taken out
    _at_least(c, {("reset_group", g): 3 for g in range(31)})
    assert E.keys(c, "pred_sfb_max") == {33, 34, 37, 38, 40, 41}
    # predictor_present 0 on a quarter, max_sfb below pred_sfb_max on a third, both window modes with M/S on
    _at_least(c, dict(adapt_no_output=30, max_sfb_below_pred=40, pred_reset_all=26))
    if channels == 2:
        _at_least(c, {("pred_ms", 0): 60, ("pred_ms", 1): 60})


FLOORS = dict(tables=_floors_tables, tns_orders=_floors_tns_orders, bands=_floors_bands, prediction=_floors_prediction)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", E.PROFILES)
def test_profile_is_finite_and_not_vacuous(pkg, oracle, profile, channels):
    coeffs, tools = E.frames(pkg, profile, channels)
    assert tools.shape == E.shape(profile)
    c = E.tools_counts(tools, channels)                            # (asserts the tables' shape on every record)
    FLOORS[profile](c, channels)
    for state in {"pns_main"} | {st for p, st in E.CASES if p == profile}:     # (every state the GPU test runs)
        for t, (out, rs, pred) in enumerate(E.oracle_chain(pkg, oracle, profile, channels, state)):
            assert np.isfinite(out).all() and (pred is None or np.isfinite(pred).all()), (state, t)
    chain = E.oracle_chain(pkg, oracle, profile, channels, "pns_main")
    rs0, _ = E.start_state(pkg, tools.shape[0], channels, "pns_main")
    assert not np.array_equal(chain[-1][1], rs0)
    assert (chain[-1][2][..., 2] > 1).any()                        # var0 > 1: predictors adapted


def test_tns_orders_fill_whole_waves(pkg):
    """k_tns picks its order template for a whole wave: the run holds waves of orders <= 7 only, waves whose largest
    order is 8 .. 12, and waves with low, middle and high orders side by side -- in the order of the streams form
    ([S][T] flat) and in that of the batch form (one position of every stream), mono and stereo"""
    _, tools = E.frames(pkg, "tns_orders")
    for channels in (1, 2):
        streams = E.tns_wave_classes(tools.reshape(-1), channels)
        _at_least(streams, {"low": 1, "mid": 1, "high": 4, "low+mid+high": 4})
        low = E.tns_wave_classes(tools[:, 6], channels)
        assert low["low"] >= 1 and low["high"] == 0
        mid = E.tns_wave_classes(tools[:, 7], channels)
        assert mid["mid"] >= 1 and mid["high"] == 0
        assert sum(E.tns_wave_classes(tools[:, t], channels)["low+mid+high"] for t in range(6)) >= 4
    # the runs the waves come from: >= 22 adjacent frames of one kind in either form, every order of them in its range
    S, T = tools.shape

    def longest(kinds, kind):
        best = cur = 0
        for x in kinds:
            cur = cur + 1 if x == kind else 0
            best = max(best, cur)
        return best
    flat = [E.order_class(s, k) for s in range(S) for k in range(T)]
    assert longest(flat, "low") >= 22 and longest(flat, "mid") >= 22
    assert longest([E.order_class(s, 6) for s in range(S)], "low") >= 22
    assert longest([E.order_class(s, 7) for s in range(S)], "mid") >= 22
    for s in range(S):
        for k in range(T):
            orders = [f[2] for c in range(2) for f in E.filter_ranges(tools[s, k]["ch"][c])]
            kind = E.order_class(s, k)
            assert kind == "mixed" or all(o <= E.TNS_LOW if kind == "low" else E.TNS_LOW < o <= E.TNS_MID
                                          for o in orders), (s, k)


def test_prediction_chains_reset_mid_chain(pkg):
    """long -> short -> long on every stream: all predictors reset inside the chain and adapt again"""
    _, tools = E.frames(pkg, "prediction")
    nw = tools["ch"]["ics"]["num_windows"][:, :, 0]
    assert (nw[:, 3] == 8).all() and (nw[:, :3] == 1).all() and (nw[:, 4:6] == 1).all() and (nw[:, 7] == 1).all()
    assert (nw[1::2, 6] == 8).all() and (nw[0::2, 6] == 1).all()


@pytest.mark.parametrize("channels", [1, 2])
def test_no_bands_leave_the_generator_alone(pkg, oracle, channels):
    """bands: a frame whose channels all have max_sfb = 0 hands the generator word back unchanged"""
    _, tools = E.frames(pkg, "bands", channels)
    chain = E.oracle_chain(pkg, oracle, "bands", channels, "pns_main")
    rs0, _ = E.start_state(pkg, tools.shape[0], channels, "pns_main")
    seen = 0
    for t in range(tools.shape[1]):
        empty = (tools["ch"]["ics"]["max_sfb"][:, t, :channels] == 0).all(axis=1)
        before = rs0 if t == 0 else chain[t - 1][1]
        assert np.array_equal(chain[t][1][empty], before[empty])
        assert (chain[t][1][~empty] != before[~empty]).mean() > 0.9          # (the others draw)
        seen += int(empty.sum())
    assert seen >= 40


def test_plain_synth_reaches_none_of_these_classes(pkg):
    """The baseline the campaign exists for: 2 000 stereo frames of synth.tools_frames hold no TNS order 13 .. 19,
    no channel above 112 bands, one num_swb per window length (one band table) and no max_sfb below 4.  A change to
    the synth that closes part of the gap fails here and is noticed."""
    synth = importlib.import_module("ffmpeg_heaac_amd.synth")
    tools = synth.tools_frames(np.random.default_rng(7 * 300 + 2), pkg, 2000, 2)
    ch = tools["ch"]
    orders = set()
    for fr in tools:
        for k in range(2):
            tns = fr["ch"][k]["tns"]
            for w in range(int(fr["ch"][k]["ics"]["num_windows"])):
                orders |= {int(o) for o in tns["order"][w][: int(tns["n_filt"][w])]}
    assert not orders & set(range(13, 20)) and 20 in orders, sorted(orders)
    nb = ch["ics"]["num_window_groups"].astype(int) * ch["ics"]["max_sfb"]
    assert nb.max() <= 112, nb.max()
    for nw in (1, 8):
        assert len(np.unique(ch["ics"]["num_swb"][ch["ics"]["num_windows"] == nw])) == 1
    assert ch["ics"]["max_sfb"].min() >= 4
    assert set(np.unique(ch["pred"]["pred_sfb_max"])) == {40}


def _dump(f, channels, coeffs, tools, rs, pred):
    S, T = tools.shape
    f.write(struct.pack("<5i", channels, S, T, rs is not None, pred is not None))
    for a in (rs, pred):
        if a is not None:
            f.write(np.ascontiguousarray(a).tobytes())
    for t in range(T):
        f.write(np.ascontiguousarray(coeffs[:, t]).tobytes())
        f.write(np.ascontiguousarray(tools[:, t]).tobytes())


def test_oracle_defined_on_tools_records(pkg):
    """the oracle on every profile, mono and stereo, with and without state, as a stand-alone program under
    AddressSanitizer + UBSan (see the module's docstring for what it found)"""
    os.makedirs(BUILD, exist_ok=True)
    odir = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(ROOT, "tests", "c", "oracle_tools.c")] + sorted(
        os.path.join(odir, f) for f in os.listdir(odir) if f.endswith(".c"))
    deps = srcs + [os.path.join(odir, "oracle.h"), os.path.join(ROOT, "include", "heaac_dsp.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-math-errno", "-ffp-contract=off",
                               "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", odir] + srcs +
                              ["-o", EXE, "-lm"])
    records = os.path.join(BUILD, "tools.bin")
    runs = frames = 0
    with open(records, "wb") as f:
        for profile in E.PROFILES:
            for channels in (1, 2):
                coeffs, tools = E.frames(pkg, profile, channels)
                for state in ("pns_main", "none"):
                    _dump(f, channels, coeffs, tools, *E.start_state(pkg, tools.shape[0], channels, state))
                    runs += 1
                    frames += tools.size
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE, records], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=env)
    os.remove(records)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    assert "runs %d, frames %d" % (runs, frames) in p.stdout, p.stdout[-500:]

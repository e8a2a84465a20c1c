"""The coupling campaign reaches what it is for (CPU, oracle only): every profile of tests/edge_coupling.py, on exactly
the records tests/test_coupling_grid_gpu.py runs, stays inside what the parser writes and holds the classes of record
it was built for -- as exact sets, not floors -- so that bit identity on the GPU says something about those classes.

The oracle's coupling is held against tests/coupling_ref.py (an independent numpy restatement shaped the other way
round) bit for bit, on every profile, mono and stereo, through the three call forms; the two int16 conversions
against two-line numpy statements on the values the GPU test converts.

test_drawn_corpus_reaches_little records the baseline: what the units of tests/test_coupling_gpu.py reach of the same
sets (one sampling index's two band tables, gain index 97 of 119, never four links, at most two slots, 132 of the
2 056 golden gains).

test_oracle_defined_on_coupling_records runs the oracle on all profiles as a stand-alone program under
AddressSanitizer + UBSan (tests/c/oracle_coupling.c).  It found nothing: on records the parser can write every read
of or_dependent_coupling and oracle_couple_after_imdct_batch is inside its record, so nothing had to be defined as
DESIGN s1 does for the stale reads of the SBR records."""
import os
import struct
import subprocess

import numpy as np
import pytest

import coupling_ref as R
import edge_coupling as K
import edge_tools as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "c", "_build")
EXE = os.path.join(BUILD, "oracle_coupling")
ALL_TABLES = {(si, nw) for si in range(E.NUM_SI) for nw in (1, 8)}
ALL_GROUPINGS = {(nswb, bits) for nswb in (12, 14, 15) for bits in range(128)}
ALL_PATTERNS = {(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)}


def _same_words(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ok = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert ok.all(), "%s: %d words differ, first at %s" % (what, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


def test_profiles_hold_exactly_what_they_are_for(pkg):
    r = {p: K.reach(K.units(pkg, p)["cce"], K.units(pkg, p)["tools"]) for p in K.PROFILES}
    for p in K.PROFILES:
        assert K.units(pkg, p)["cce"].shape[1] == K.N_CCE[p]
    t = r["tables"]
    assert t["tables"] == ALL_TABLES
    assert t["max_sfb_edge"] == {(si, nw, e) for si, nw in ALL_TABLES for e in (0, 1, "num_swb-1", "num_swb")}
    assert t["other_window"] == {(1, 1), (1, 8), (8, 1), (8, 8)}
    g = r["groupings"]
    assert g["groupings"] == ALL_GROUPINGS and max(g["last_index"]) == 119
    assert g["other_window"] == {(8, 1), (8, 8)}
    li = r["links"]
    assert li["n_links"] == {0, 1, 2, 3, 4} and li["link_patterns"] == ALL_PATTERNS
    assert li["twice"] >= 4 and li["channel1_only"] >= 4
    s = r["slots"]
    assert s["slot_counts"] == set(K.SLOT_COUNTS)
    assert s["gaps"] == 8 and s["after_between"] == 6 and s["both_points"] == 20     # (twice what SLOT_CASES lists)
    assert r["order"]["slot_counts"] == {16} and r["order"]["both_points"] == 4
    assert r["gains"]["gains"] == K.golden_words() and len(K.golden_words()) > 1900
    a = r["around_tns"]
    assert a["both_points"] == len(K.units(pkg, "around_tns")["tools"]) and a["other_window"] == {(1, 1), (1, 8), (8, 1), (8, 8)}


def test_golden_gains_stand_side_by_side():
    lists = K.golden_lists()
    flat = K.GOLDEN.ravel()
    assert set(lists.view(np.uint32).ravel()) == K.golden_words()
    big, small = np.float32(np.inf), np.float32(-np.inf)
    assert lists[0][0] == small and lists[0][1] == big
    by = lists[len(lists) // 2]
    assert abs(by[0]) == np.abs(flat).min() and np.isinf(by[1])


def test_zero_band_records_hide_a_nan_under_every_zero_band(pkg):
    u = K.units(pkg, "zero_bands")
    seen = set()
    for k in range(len(u["tools"])):
        for s in range(2):
            rec = u["cce"][k, s]
            nb = int(rec["ics"]["num_window_groups"]) * int(rec["ics"]["max_sfb"])
            bt = rec["band_type"][:nb] != 0
            for l in range(int(rec["n_links"])):
                g = rec["link"][l]["gain"]
                assert np.isnan(g[:nb][~bt]).all() and np.isnan(g[nb:]).all() and np.isfinite(g[:nb][bt]).all()
            seen.add("all_zero" if not bt.any() else "none_zero" if bt.all() else
                     "first_only" if bt.sum() == 1 and bt[0] else "last_only" if bt.sum() == 1 and bt[-1] else
                     "alternating" if (bt[::2].all() and not bt[1::2].any()) or (bt[1::2].all() and not bt[::2].any())
                     else "?")
    assert seen == set(K.ZERO_PATTERNS)


def test_around_tns_filters_run_on_the_coupled_bands(pkg):
    """every target filter of around_tns runs (size > 0) at order 20, 12 or 7 in both directions, and both coupling
    elements write lines inside it"""
    u = K.units(pkg, "around_tns")
    seen = set()
    for k in range(len(u["tools"])):
        for c in range(2):
            ch = u["tools"][k]["ch"][c]
            ranges = E.filter_ranges(ch)
            assert ranges and all(f[7] > 0 for f in ranges)
            seen |= {(int(ch["ics"]["num_windows"]), f[2], f[3]) for f in ranges}
            lines = np.zeros(1024, bool)
            for (w, _, _, _, _, _, start, size) in ranges:
                lines[128 * w + start: 128 * w + start + size] = True
            for point in (K.BEFORE_TNS, K.BETWEEN):
                adds = K.contributions(u, k, c, point)
                assert len(adds) == 1 and (adds[0][lines] != 0).any()
        assert (u["tools"][k]["ch"][0]["band_type"][:8] == E.NOISE_BT).any()
        assert u["tools"][k]["ms_present"] and u["tools"][k]["common_window"]
    assert seen == {(nw, o, d) for nw in (1, 8) for o in K.TNS_TEMPLATE_ORDERS for d in (0, 1)}


def test_order_profile_does_not_associate(pkg):
    assert K.order_property(pkg) >= 2000
    for j in range(40):
        assert 12 <= abs(K.order_exponents(j + 1) - K.order_exponents(j)) <= 24


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", K.PROFILES)
def test_restatement_equals_oracle(pkg, oracle, profile, channels):
    """tests/coupling_ref.py against the oracle through the three call forms; results finite except in `gains`
    (+-inf gains, no NaN), and no NaN anywhere: the NaN gains and spectra of the records are never read"""
    u = K.units(pkg, profile, channels)
    first = None
    for form in K.FORMS:
        ref = K.oracle_run(pkg, oracle, profile, channels, form)
        got = K.run_forms(R.spectral_tools_batch_ex, (R.PRE, R.POST, R.PRE | R.POST), channels, u, form)
        _same_words(got[0], ref[0], form + " coefficients")
        assert np.array_equal(got[1], ref[1]), form + " generator"
        assert not np.isnan(ref[0]).any()
        assert profile == "gains" or np.isfinite(ref[0]).all()
        if form == "all":
            first = ref
            # noise bands: the generator moved (`order` has none: nothing but the sums)
            assert np.array_equal(ref[1], u["rng"]) == (profile == "order")
        elif form == "pre_post":
            assert np.array_equal(ref[0].view(np.uint32), first[0].view(np.uint32)) and np.array_equal(ref[1], first[1])
        else:
            assert np.array_equal(ref[1], u["rng"])
    # coupling really happened: the result differs from the tools without it
    plain = oracle.spectral_tools_batch_ex(channels, oracle.TOOLS_ALL, u["coeffs"], u["tools"], rng=u["rng"])[0]
    differs = (plain.view(np.uint32) != first[0].view(np.uint32)).any(axis=(1, 2))
    assert differs.mean() > 0.6, differs.mean()


def _couple_cases(pkg):
    for channels in (1, 2):
        for on in ((0, 0), (1, 0), (0, 1), (1, 1)):
            for n in (1, 2, 257):
                yield "ch%d on%d%d n%d" % (channels, on[0], on[1], n), channels, K.couple_case(pkg, n, channels, on)
    yield "golden", 2, K.couple_golden(pkg)


def test_independent_restatement_equals_oracle(pkg, oracle):
    """apply_independent_coupling restated against oracle.couple_after_imdct_batch on the records of the GPU test:
    three chained calls, float words and int16; the sums of frame 0 land on, inside and outside both int16 limits"""
    for what, channels, (pcm, steps) in _couple_cases(pkg):
        ref = got = pcm
        for k, (cce, cpl) in enumerate(steps):
            ref, r16 = oracle.couple_after_imdct_batch(channels, ref, cce, cpl, s16=True)
            got, g16 = R.couple_after_imdct_batch(channels, got, cce, cpl, s16=True)
            _same_words(got, ref, "%s call %d" % (what, k))
            assert np.array_equal(g16, r16), (what, k)
            assert not np.isnan(ref).any()
            if k == 0 and what != "golden":
                for c in range(channels):
                    if steps[0][1]["on"][0, c]:
                        assert r16[0, :6, c].tolist() == [32766, 32767, 32767, -32768, -32768, -32767], what
                        assert ref[0, c, 1] == K.S16_TOP and ref[0, c, 4] == 384.0
    pcm, steps = K.couple_golden(pkg)
    used = set()
    for cce, cpl in steps:
        used |= set(int(x) for x in cpl["gain"].view(np.uint32).ravel())
    assert used == K.golden_words()


@pytest.mark.parametrize("sse2", [False, True])
def test_conversions_restated(oracle, sse2):
    """the two float -> int16 conversions as two lines of numpy each, against the oracle on the values the GPU test
    converts; on the C path every float 385 + k / 32768 gives k"""
    vals = np.concatenate([K.interleave_pool(sse2, 70000), K.interleave_edges(sse2)])
    want = oracle.float_to_int16_interleave([vals], sse2=sse2)[:, 0]
    assert np.array_equal((R.s16_sse2 if sse2 else R.s16_c)(vals), want)
    if not sse2:
        every = oracle.float_to_int16_interleave([K.c_path_values()])[:, 0]
        assert np.array_equal(every.astype(np.int64), np.arange(-32768, 32768))
        edge = dict(zip(K.interleave_edges(False)[:4].tolist(),
                        oracle.float_to_int16_interleave([K.interleave_edges(False)[:4]])[:, 0].tolist()))
        assert sorted(edge.values()) == [-32768, -32768, 32767, 32767], edge
    else:
        ties = (np.arange(-6, 6) + 0.5).astype(np.float32)
        assert oracle.float_to_int16_interleave([ties], sse2=True)[:, 0].tolist() == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6]
        ends = np.array([32767.5, -32767.5, 32768.0, -32768.0, np.inf, -np.inf, np.nan], np.float32)
        assert oracle.float_to_int16_interleave([ends], sse2=True)[:, 0].tolist() == [32767, -32768, 32767, -32768,
                                                                                        -32768, -32768, -32768]


def test_interleave_planes_are_what_the_docstring_says():
    kinds = set()
    for channels in range(1, 17):
        for length in (4, 12, 1024, 2048):
            for n in (1, 2, 65):
                planes, size = K.interleave_planes(channels, length, n)
                assert len(planes) == channels
                for c, (o, s) in enumerate(planes):
                    kinds.add("stride0" if s == 0 else "pair" if s == 2 * length else "wide" if s > length else "tight")
                    kinds.add("twice") if c and planes[c - 1] == (o, s) else None
                if length >= 1024:                                  # every edge of either conversion is converted
                    for sse2 in (False, True):
                        host = K.interleave_pool(sse2, size)
                        read = np.concatenate([host[o: o + length] for o, _ in planes]).view(np.uint32)
                        assert set(K.interleave_edges(sse2).view(np.uint32)) <= set(read), (channels, length, n, sse2)
    assert kinds == {"stride0", "pair", "wide", "tight", "twice"}
    # n * len / 4 lanes: partly filled last blocks with live neighbours, and a single partly filled block
    assert (65 * 4 // 4) % 256 == 65 and (65 * 12 // 4) % 256 == 195 and (2 * 1024 // 4) % 256 == 0


DRAWN = [(False, False, False), (True, False, False), (True, True, False), (False, True, True)]


def test_drawn_corpus_reaches_little(pkg):
    """What the units of tests/test_coupling_gpu.py (its four parameter sets, 24 units each) reach of the sets above:
    a measurement, asserted so that a change to those draws is noticed."""
    import test_coupling_gpu as G
    got = None
    for cpe, behind, two in DRAWN:
        rng = np.random.default_rng(900 + 4 * cpe + 2 * behind + two)
        _, u = G._units(pkg, rng, 3, 2, cpe, 24, behind, [0, 1], two)
        r = K.reach(u["cce"], u["tools"])
        if got is None:
            got = r
        else:
            for k, v in r.items():
                got[k] = got[k] | v if isinstance(v, set) else got[k] + v
    tables = {t for t in got["tables"]}
    print("drawn corpus:", {k: (len(v) if isinstance(v, set) else v) for k, v in got.items()},
          sorted(got["slot_counts"]), sorted(got["n_links"]), max(got["last_index"]), sorted(tables))
    assert tables == {(3, 1), (3, 8), (4, 8), (5, 8)}      # sampling index 3; 4 and 5 share its short table
    assert got["slot_counts"] <= {1, 2} and got["n_links"] <= {1, 2}
    assert not got["link_patterns"] and max(got["last_index"]) < 119
    assert got["gaps"] == 0 and got["after_between"] == 0
    assert len(got["gains"] & K.golden_words()) < len(K.golden_words()) // 8
    assert DRAWN_REACH == dict(tables=len(tables), groupings=len(got["groupings"] & ALL_GROUPINGS),
                               last_index=max(got["last_index"]), slot_counts=sorted(got["slot_counts"]),
                               n_links=sorted(got["n_links"]), gains=len(got["gains"] & K.golden_words()),
                               both_points=got["both_points"])


# of 26 tables, 384 groupings with max_sfb = num_swb, gain index 119, 16 patterns of four links (none: never four links),
# slot counts {1, 2, 15, 16}, 2056 golden gains; both spectral points in 12 of the 96 units
DRAWN_REACH = dict(tables=4, groupings=6, last_index=97, slot_counts=[1, 2], n_links=[1, 2], gains=132, both_points=12)


def _dump_dependent(f, channels, u, form):
    n, k = u["cce"].shape
    f.write(struct.pack("<6i", 0, channels, n, k, form, 0))
    for a in (u["rng"], u["coeffs"], u["tools"], u["cce"], u["cce_coeffs"]):
        f.write(np.ascontiguousarray(a).tobytes())


def test_oracle_defined_on_coupling_records(pkg):
    """the oracle's dependent coupling on every profile, mono and stereo, through the three call forms, and its
    independent coupling on the records of the GPU test, as a stand-alone program under AddressSanitizer + UBSan (see
    the module's docstring for what it found)"""
    os.makedirs(BUILD, exist_ok=True)
    odir = os.path.join(ROOT, "oracle")
    srcs = [os.path.join(ROOT, "tests", "c", "oracle_coupling.c")] + sorted(
        os.path.join(odir, f) for f in os.listdir(odir) if f.endswith(".c"))
    deps = srcs + [os.path.join(odir, "oracle.h"), os.path.join(ROOT, "include", "heaac_dsp.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-math-errno", "-ffp-contract=off",
                               "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", odir] + srcs +
                              ["-o", EXE, "-lm"])
    records = os.path.join(BUILD, "coupling.bin")
    runs = frames = 0
    with open(records, "wb") as f:
        for profile in K.PROFILES:
            for channels in (1, 2):
                u = K.units(pkg, profile, channels)
                for form in range(3):
                    _dump_dependent(f, channels, u, form)
                    runs += 1
                    frames += len(u["tools"])
        for what, channels, (pcm, steps) in _couple_cases(pkg):
            f.write(struct.pack("<6i", 1, channels, len(pcm), len(steps), 0, 1))
            f.write(np.ascontiguousarray(pcm).tobytes())
            for cce, cpl in steps:
                f.write(np.ascontiguousarray(cce).tobytes())
                f.write(np.ascontiguousarray(cpl).tobytes())
            runs += 1
            frames += len(pcm)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE, records], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=env)
    os.remove(records)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    assert "runs %d, frames %d" % (runs, frames) in p.stdout, p.stdout[-500:]
    assert ": 0 NaN words" in p.stdout and not [ln for ln in p.stdout.splitlines() if "NaN words" in ln and
                                                 not ln.endswith(": 0 NaN words")], p.stdout[-2000:]


def test_every_interleave_kernel_is_built(pkg):
    """heaac_pcm_interleave_batch dispatches on the channel count; a count whose packed kernel is missing from the
    dispatch falls through to k_interleave, which writes the same words -- no comparison of outputs can see that.
    So the library is asked: the host stubs of all 16 k_interleave_packed<format, 1 .. 8> instantiations, of both
    k_interleave<format> and of the four k_couple<channels, int16> are in it (an instantiation exists only where a
    launch names it)."""
    with open(pkg.LIB_PATH, "rb") as f:
        blob = f.read()
    fmts = (pkg.PCM_S16, pkg.PCM_S16_SSE2)
    for fmt in fmts:
        for ch in range(1, 9):
            assert blob.find(b"k_interleave_packedILi%dELi%dEE" % (fmt, ch)) >= 0, "k_interleave_packed<%d, %d>" % (fmt, ch)
        assert blob.find(b"k_interleaveILi%dEE" % fmt) >= 0, "k_interleave<%d>" % fmt
    for ch in (1, 2):
        for s16 in (0, 1):
            assert blob.find(b"k_coupleILi%dELb%dEE" % (ch, s16)) >= 0, "k_couple<%d, %d>" % (ch, s16)

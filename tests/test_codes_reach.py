"""The parsers' structural campaign on the CPU (tests/edge_codes.py): REACH -- what the corpora emit is, as exact sets,
every codeword of the scalefactor book, the eleven spectral books, the ten SBR and the ten Parametric Stereo books, every
escape length and every section and accumulator case, while the drawn corpora the other parser tests use stay at 13
scalefactor codes of 121; VALUES -- every taken unit through the host parser comes back as the writers' models state it,
field for field, every refused one gives its status and leaves the stream state as it was; WALKS -- the same corpora
through the host instantiations of the device walks (one-unit forms and the streams forms at T = 1 and T = 3) against
the host parser, every output pre-filled."""
import numpy as np
import pytest

import edge_codes as EC
import parse_device_common as PC
import parse_streams_common as PS
import sbr_bitwriter as SW
import sbr_device_common as SD
import test_parse as TP
import test_sbr_parse as TS


# ---- reach ----
def test_aac_books_escapes_sections_and_ends_are_reached_whole():
    units, em, tally = EC.aac_units()
    assert em.sf == set(range(-60, 61))
    for eight in (False, True):
        for chain in ("spectral", "noise", "intensity"):
            assert tally[(chain, eight)] == set(range(-60, 61)), (chain, eight)
    for book, size in EC.BOOK_SIZE.items():
        assert em.spec[book] == set(range(size)), book
    import aac_bitwriter as W
    assert sum(EC.BOOK_SIZE.values()) == len(W.T["aac_spec_code"]) == 1241      # the books as the table text holds them
    assert [W.T["aac_spec_first"][b] - W.T["aac_spec_first"][b - 1] for b in range(1, 12)] == list(EC.BOOK_SIZE.values())
    for book, count in EC.SIGN_PATTERNS.items():
        assert len(em.signed[book]) == count, book
    # the zero-line sign cases of the unsigned quad books and of book 11: a zero line in front of a negative one
    assert (0, -1, 0, 0) in em.signed[3] and (0, 0, 0, -2) in em.signed[4] and (0, -16) in em.signed[11] and (0, -3) in em.signed[11]
    want = set()
    for n in range(9):
        for v in (1 << (n + 4), (1 << (n + 5)) - 1):
            for neg in (False, True):
                want |= {(n, v, neg, 0, False), (n, v, neg, 1, False), (n, v, neg, 0, True), (n, v, neg, 1, True)}
    assert want <= em.esc and (9, 8192, False, 0, False) in em.esc
    assert {n for n, *_ in em.esc} == set(range(10))
    cases = [u["case"] for u in units if u["profile"] == "sections"]
    assert {c for c in cases if c != "run_past_max_sfb"} == {("long", 30), ("long", 31), ("long", 32), ("long", 51),
                                                          ("long", "equal_neighbours"), ("short", (6, 7, 8, 14, 15, 7, 14, 15))}
    assert cases.count("run_past_max_sfb") == 2
    ends = {u["case"]: u["status"] for u in units if u["profile"] == "sf_ends"}
    for e in ("long", "short"):
        for chain in ("spectral", "noise", "intensity", "global_gain"):
            assert (ends[(chain, 0, e)], ends[(chain, 255, e)], ends[(chain, -1, e)], ends[(chain, 256, e)]) == (0, 0, -1, -1)
        assert [ends[("noise_start", v, e)] for v in (0, 255, -1, 256, -91)] == [0, 0, -1, -1, -1]
    starts = {(u["exp"]["ch"][-1]["noise_start"], u["case"][1]) for u in units if u["profile"] == "sf_ends" and u["case"][0] == "noise_start"}
    assert {(511, 255), (511, 256), (0, -91)} <= starts
    assert sorted(EC.aac_groups(units)) == GROUPS
    assert {u["cpe"] for u in units} == {False, True} and {u["exp"].get("common_window") for u in units} == {None, 0, 1}
    assert sum(u["status"] != 0 for u in units) == 2 * 11 + 1 + 2      # eleven landings outside per window, the ninth escape length, two runs


def test_sbr_and_ps_books_are_reached_whole(pkg):
    streams, em = EC.he_streams(pkg)
    for t in SW.SBR_T + SW.PS_T:
        assert em.huff[t] == set(range(len(SW.T[t][0]))), t
    assert sum(len(SW.T[t][0]) for t in SW.SBR_T) == 604 and sum(len(SW.T[t][0]) for t in SW.PS_T) == 242
    # time deltas through both index mappings (low -> high and high -> low resolution), and without a change
    classes = set().union(*[s["classes"] for s in streams if s["kind"][0] == "sbr_books"])
    assert {("env", "time", 0, 1), ("env", "time", 1, 0), ("env", "time", 0, 0), ("env", "time", 1, 1), ("env", "freq"),
            ("noise", "time"), ("noise", "freq")} <= classes
    # every PS book whole at every band count: IID 10 / 20 / 34 coarse and fine, ICC 10 / 20 / 34, IPD / OPD 5 / 11 / 17
    ps = [s for s in streams if s["kind"][0] == "ps_books"]
    assert [s["kind"][1] for s in ps] == list(range(6))
    for s in ps:
        fine = s["kind"][1] >= 3
        mine = EC.PS_TABLES[fine] + ("icc_df", "icc_dt", "ipd_df", "ipd_dt", "opd_df", "opd_dt")
        for t in SW.PS_T:
            assert s["emitted"].huff[t] == (set(range(len(SW.T[t][0]))) if t in mine else set()), (s["kind"], t)
        for t in mine[1::2]:
            assert {(t, "envelope border"), (t, "frame border")} <= s["classes"], (s["kind"], t)
    assert {(s["exp"]["ps"]["nr_iid_par"][0], s["exp"]["ps"]["nr_ipdopd_par"][0]) for st in ps for s in st["frames"]} == {(10, 5), (20, 11), (34, 17)}
    # and whole in the frames the walks and the device parsers are handed: every frame but the first of its stream, which
    # carries the header -- per channel configuration, as exact sets per book (nothing of a book the configuration has not)
    for cpe in (False, True):
        items = EC.HeItems(pkg, streams, cpe)
        assert all(t > 0 for _, t in items.items)
        handed = EC.symbols_handed(items, items.items, [1] * len(items.items))
        whole = EC.books_of(cpe)
        for t in SW.SBR_T + SW.PS_T:
            assert handed[t] == whole.get(t, set()), (cpe, t)
    ends = {s["kind"][1:] for s in streams if s["kind"][0] == "sbr_ends"}
    assert len(ends) == 12 and {k[2] for k in ends} == {"env", "noise"} and {k[3] for k in ends} == {7, 6, 5}
    for s in streams:
        if s["kind"][0] == "sbr_ends":
            assert [f["status"] for f in s["frames"]].count(EC.ERR_DATA) == 1


def test_the_drawn_corpora_stay_in_a_corner_of_the_books(pkg):
    """The baseline this campaign was written against: the corpora the other parser tests draw (parse_device_common.
    in_scope_steps, sbr_device_common.he_units) send the 13 scalefactor deltas -6 .. 6 of 121 -- random_ics draws no
    others -- and a part of the SBR and PS books."""
    rng = np.random.default_rng(123)
    with EC.counting() as em:
        for cpe, aot, si in [(False, 2, 3), (True, 2, 3), (True, 1, 4), (False, 2, 6)]:
            PC.in_scope_steps(rng, si, aot, cpe, 30, 2, adts=0.3, sbr=0.3)
        for cpe, ps_modes in SD.STREAMS:
            writers = SD.make_writers(pkg, 6, cpe, ps_modes)
            for _ in range(5):
                SD.he_units(rng, writers, cpe)
    assert em.sf == set(range(-6, 7))
    assert len(em.sf) == 13 and len(SW.T["t_env_15"][0]) == 121
    for t in ("f_env_15", "f_env_30", "f_env_bal_15", "f_env_bal_30", "iid_dt1", "iid_dt0", "icc_dt"):
        assert len(em.huff[t]) < len(SW.T[t][0]) // 2, (t, len(em.huff[t]))
    # and the emit functions are the writers' own again
    import aac_bitwriter as W
    assert W.put_sf.__module__ == "aac_bitwriter" and SW.Bits.huff.__module__ == "sbr_bitwriter"


# ---- values: the host parser against the writers' models ----
GROUPS = [(3, 2, False), (3, 2, True), (5, 2, False), (6, 2, False)]      # (si, aot, cpe) of the corpus, held below


@pytest.mark.parametrize("si,aot,cpe", GROUPS)
def test_aac_units_come_back_as_the_writer_states_them(pkg, si, aot, cpe):
    units = EC.aac_groups(EC.aac_units()[0])[(si, aot, cpe)]
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    cc = 2 if cpe else 1
    st = np.zeros(len(units), pkg.AAC_STREAM_DT)
    st["window_sequence"] = 3
    before = st.copy()
    out = PC.host_parse(pkg, cfg, st, [u["au"] for u in units], cc)
    for f, u in enumerate(units):
        e = u["exp"]
        assert int(out["status"][f]) == u["status"], (u["profile"], u["case"], int(out["status"][f]))
        if u["status"]:
            # each of these refusals is the reference's own, made behind decode_ics_info: the channels' window history
            # has moved on to the refused unit's and the element's tag is mapped, as include/heaac_parse.h states and
            # test_aac_parse_refusal_state.py pins; nothing else of the stream state moves (the device walks, which defer
            # such a unit, leave every byte: parse_device_common.compare)
            assert out["info"][f]["refused"] & pkg.REFUSED_AS_REFERENCE and out["info"][f]["channels"] == 0
            want = before[f].copy()
            for c, d in enumerate(e["ch"]):
                want["window_sequence"][c], want["use_kb_window"][c] = d["window_sequence"], d["window_shape"]
            want["mapped_tag"] = 1
            assert st[f].tobytes() == want.tobytes(), (u["profile"], u["case"])
            continue
        assert out["info"][f]["channels"] == e["channels"] and out["info"][f]["bits_consumed"] == e["bits"]
        assert out["info"][f]["sbr_payload_bit"] == -1
        if cpe:
            assert out["tools"][f]["common_window"] == e["common_window"] and out["tools"][f]["ms_present"] == 0
            assert not out["tools"][f]["ms_mask"].any()
        for c, d in enumerate(e["ch"]):
            TP._check_channel(out, f, c, d, e["sf"][c], si)
    taken = [u for u in units if not u["status"]]
    assert np.isfinite(out["coeffs"][[not u["status"] for u in units]]).all() and len(taken) > 0


@pytest.mark.parametrize("cpe", [False, True])
def test_he_frames_come_back_as_the_writer_states_them(pkg, cpe):
    streams, _ = EC.he_streams(pkg)
    items = EC.HeItems(pkg, streams, cpe)
    refused = 0
    for s, rec in zip(items.streams, items.host):
        for t, (f, h) in enumerate(zip(s["frames"], rec)):
            what = (s["kind"], t)
            assert h["status"] == f["status"], (what, h["status"])
            if f["status"]:
                # what test_sbr_parse.py::test_malformed_grids_drop_the_element_and_keep_the_stream states: the frame is
                # switched off, the channel data rolled back (start, reset and the "old" range may move)
                refused += 1
                assert h["sbr"]["start"][0] == 0, what
                assert (h["sst_after"] != h["sst"]).sum() <= 4, what
                continue
            exp = f["exp"]
            exp["sbr"]["hdr"] = h["sbr"]["hdr"]
            assert items.tab.headers()[int(h["sbr"]["hdr"][0])].tobytes() == exp["hdr"][0].tobytes(), what
            TS._same(h["sbr"], exp["sbr"], "%s sbr" % (what,))
            if not cpe:
                TS._same(h["ps"], exp["ps"], "%s ps" % (what,))
    assert refused == 6                                            # three fields a channel configuration, both ends


# ---- walks on the host ----
def _host_call(pkg):
    def call(cfg, st, rows, cc, sst, hdr, with_ps):
        T, S = len(rows), len(rows[0])
        after = st.copy()
        got = pkg.parse_core_streams(cfg, after, PS.flat(rows), T, coeff_channels=cc, sst_in=sst, hdr=hdr, with_ps=with_ps,
                                     out=PS.filled_streams(pkg, S, T, cc, sst, with_ps))
        return got, after
    return call


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("si,aot,cpe", GROUPS)
def test_aac_units_through_the_walks_on_the_host(pkg, si, aot, cpe, T):
    units = EC.aac_groups(EC.aac_units()[0])[(si, aot, cpe)]
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    S = -(-len(units) // T)
    picks = EC.spread(len(units), S * T, 11)
    rows = [[units[picks[s * T + t]]["au"] for s in range(S)] for t in range(T)]
    st = np.zeros(S, pkg.AAC_STREAM_DT)
    st["window_sequence"] = np.random.default_rng(5).integers(0, 4, (S, 2))
    for cc in ((2,) if cpe else (1, 2)):
        got = EC.run_walk(pkg, PS.HostOne(pkg), _host_call(pkg), cfg, st, rows, cc)
        want = [([units[picks[s * T + t]]["status"] != 0 for t in range(T)] + [True]).index(True) for s in range(S)]
        assert got["taken"].astype(int).tolist() == want           # a lane stops at its first refused unit, and only there


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("cpe", [False, True])
def test_he_frames_through_the_walks_on_the_host(pkg, cpe, T):
    streams, _ = EC.he_streams(pkg)
    items = EC.HeItems(pkg, streams, cpe)
    picks = items.items if T == 1 else [(k, t) for k, t in items.items if t % T == 1]
    picks = [picks[i] for i in EC.spread(len(picks), len(picks), 12)]
    rows, st, sst = items.rows(picks, T)
    got = EC.run_walk(pkg, PS.HostOne(pkg), _host_call(pkg), items.cfg, st, rows, items.cc, sst, items.tab.headers(),
                      items.with_ps, items.tab)
    want = []
    for k, t in picks:                                             # a lane stops at its first refused frame, or at its stream's end
        fr = items.streams[k]["frames"][t:t + T]
        want.append(([f["status"] != 0 for f in fr] + [True]).index(True))
    assert got["taken"].astype(int).tolist() == want
    if T == 1:                                                     # every codeword was in a frame this call took
        handed = EC.symbols_handed(items, picks, got["taken"])
        assert all(handed[t] == syms for t, syms in EC.books_of(cpe).items())

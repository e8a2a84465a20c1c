"""The parsers' structural campaign on the GPU (tests/edge_codes.py): the corpora that reach every codeword of every
code book, every escape length and every accumulator end through heaac_aac_parse_device, heaac_sbr_parse_device,
heaac_heaac_parse_device and the two *_device_streams calls at T = 1 and T = 3, byte for byte against the host parser
through the comparisons the other device-parser tests use, every output pre-filled.  Sizes 1, 63, 64 and 65 (two
blocks: the LDS copy of the tables is made twice); the units are permuted so that one wave holds the 1-bit codes next
to the 19- and 20-bit ones and refused units next to taken ones.  Then bytes to PCM for the scalefactor and escape
units."""
import numpy as np
import pytest

import edge_codes as EC
import parse_device_common as PC
import sbr_device_common as SD
import test_parse as TP
import test_parse_streams_gpu as G

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65]


def _dev_call(pkg, dev):
    def call(cfg, st, rows, cc, sst, hdr, with_ps):
        got, after, _ = G.streams_call(pkg, dev, cfg, st, rows, cc, sst, hdr, with_ps)
        return got, after
    return call


@pytest.mark.parametrize("S", SIZES)
def test_aac_corpora_on_the_gpu(pkg, dev, S):
    """Every configuration of the corpus at T = 1 and T = 3: the one-unit device call position by position against
    the host parser, the streams call against that and against the host parser's chain."""
    groups = EC.aac_groups(EC.aac_units()[0])
    for j, (si, aot, cpe) in enumerate(sorted(groups)):
        units = groups[(si, aot, cpe)]
        cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
        for T in (1, 3):
            picks = EC.spread(len(units), S * T, 100 * S + 10 * j + T)
            rows = [[units[picks[s * T + t]]["au"] for s in range(S)] for t in range(T)]
            st = np.zeros(S, pkg.AAC_STREAM_DT)
            st["window_sequence"] = np.random.default_rng(S).integers(0, 4, (S, 2))
            got = EC.run_walk(pkg, G.DevOne(pkg, dev), _dev_call(pkg, dev), cfg, st, rows, 2 if cpe else 1 + (S & 1))
            want = [([units[picks[s * T + t]]["status"] != 0 for t in range(T)] + [True]).index(True) for s in range(S)]
            assert got["taken"].astype(int).tolist() == want
            if S >= 63 and si == 3:
                sizes = [len(a) for a in rows[0]]
                assert max(sizes) > 4 * min(sizes) and 0 < sum(w == 0 for w in want) < S      # one wave, very different lanes
            if S * T >= len(units):
                assert set(picks) == set(range(len(units)))                                   # the whole corpus in this call


_ITEMS = {}


def _items(pkg, cpe):
    if cpe not in _ITEMS:
        _ITEMS[cpe] = EC.HeItems(pkg, EC.he_streams(pkg)[0], cpe)
    return _ITEMS[cpe]


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("cpe", [False, True])
def test_he_corpora_on_the_gpu(pkg, dev, cpe, S):
    """Frames of every chain, each lane from the states the host parser held in front of its frame: at S = 65 and T = 3
    every frame of the corpus is in the call."""
    items = _items(pkg, cpe)
    for T in (1, 3):
        pool = items.items if T == 1 or S < 63 else [(k, t) for k, t in items.items if t % T == 1]
        picks = [pool[i] for i in EC.spread(len(pool), S, 200 * S + T + cpe)]
        rows, st, sst = items.rows(picks, T)
        got = EC.run_walk(pkg, G.DevOne(pkg, dev), _dev_call(pkg, dev), items.cfg, st, rows, items.cc, sst, items.tab.headers(),
                          items.with_ps, items.tab)
        want = []
        for k, t in picks:
            fr = items.streams[k]["frames"][t:t + T]
            want.append(([f["status"] != 0 for f in fr] + [True]).index(True))
        assert got["taken"].astype(int).tolist() == want
        if S == 65 and T == 3:
            assert len(pool) <= S and {(k, t + j) for k, t in picks for j in range(T)} >= set(items.items)
            handed = EC.symbols_handed(items, picks, got["taken"])         # every codeword was in a frame the call TOOK
            assert all(handed[t] == syms for t, syms in EC.books_of(cpe).items())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cpe", [False, True])
def test_he_corpora_through_the_combined_call(pkg, dev, cpe, n):
    """heaac_heaac_parse_device over every frame of the corpus in calls of n (n = 1: the first five frames of the
    permuted corpus, one a call): status, records and SBR states as the host parser's, the AAC state of every unit taken
    as well; every output pre-filled.  Over the calls of one size every codeword is in a unit the call took."""
    import torch
    items = _items(pkg, cpe)
    order = [items.items[i] for i in EC.spread(len(items.items), len(items.items), 31 + n)]
    if n == 1:
        order = order[:5]
    d_hdr = pkg.to_device(items.tab.headers())
    handed = []
    for at in range(0, len(order), n):
        picks = order[at:at + n]
        m = len(picks)
        rows, st, sst = items.rows(picks, 1)
        aus = rows[0]
        st_host, sst_host = st.copy(), sst.copy()
        host = SD.host_parse(pkg, items.cfg, st_host, sst_host, items.tab, aus, items.cc, items.with_ps)
        d_au, d_off = G.load(pkg, aus)
        d_st = pkg.to_device(st.copy())
        pre = {k: pkg.to_device(v) for k, v in PC.filled(pkg, m, items.cc).items()}
        he = {k: (pkg.to_device(v) if v is not None else None) for k, v in SD.filled(pkg, sst, m, items.with_ps).items()}
        out = dev.heaac_parse_device(items.cfg, d_st, pkg.to_device(sst), d_au, d_off, d_hdr, coeff_channels=items.cc,
                                     sst_out=he["sst"].view(-1), sbr=he["sbr"], ps=he["ps"],
                                     status=torch.full((m,), 7, dtype=torch.int32, device="cuda"), **pre)
        torch.cuda.synchronize()
        got = dict(sst=out["sst"].cpu().numpy().reshape(m, -1), sbr=out["sbr"].cpu().numpy().view(pkg.SBR_FRAME_DT),
                   ps=out["ps"].cpu().numpy().view(pkg.PS_FRAME_DT) if items.with_ps else None, status=out["status"].cpu().numpy())
        ok = SD.compare(pkg, host, sst_host, sst, got)
        assert ok.tolist() == [items.streams[k]["frames"][t]["status"] == 0 for k, t in picks]
        assert np.array_equal(PC.rows(out["info"].cpu().numpy().view(pkg.AAC_INFO_DT), m)[ok], PC.rows(host["info"], m)[ok])
        assert np.array_equal(PC.rows(d_st.cpu().numpy(), m)[ok], PC.rows(st_host, m)[ok])
        handed.append(EC.symbols_handed(items, picks, ok))
    if n > 1:
        assert all(set().union(*[h[t] for h in handed]) == syms for t, syms in EC.books_of(cpe).items())


@pytest.mark.parametrize("cpe", [False, True])
def test_scalefactor_and_escape_units_from_bytes_to_pcm(pkg, oracle, dev, cpe):
    """bytes -> heaac_aac_parse_device -> heaac_spectral_tools_batch -> heaac_lc_decode_batch for the taken units of
    sf_book and escapes (every scalefactor code on every chain, every escape length): float32 PCM bit for bit as the
    oracle's from the host-parsed records; the largest coefficients stay finite."""
    import torch
    units = [u for u in EC.aac_groups(EC.aac_units()[0])[(3, 2, cpe)] if u["profile"] in ("sf_book", "escapes") and not u["status"]]
    n, chn = len(units), 2 if cpe else 1
    assert n >= 5
    cfg = TP._cfg(pkg, 2, 3, chn)
    aus = [u["au"] for u in units]
    st = np.zeros(n, pkg.AAC_STREAM_DT)
    host = pkg.aac_parse_batch(cfg, st, aus)
    assert host["failed"] == 0
    ref_rng = np.full(n, 0x1f2e3d4c, np.int32)
    ref_c, ref_rng = oracle.spectral_tools_batch(chn, np.ascontiguousarray(host["coeffs"][:, :chn]), host["tools"], rng=ref_rng)
    ref_pcm, ref_state = oracle.lc_decode_batch(chn, ref_c, np.ascontiguousarray(host["ics"][:, :chn]), np.zeros((n, 512 * chn), np.float32), oracle.PCM_F32)
    assert np.isfinite(ref_c).all() and np.isfinite(ref_pcm).all() and np.abs(ref_pcm).max() > 0
    assert np.abs(host["coeffs"]).max() > 8191.0 ** (4.0 / 3.0) * 2.0 ** -21      # the largest escape value is in there
    buf, off = pkg.pack_units(aus)
    d_st = pkg.to_device(np.zeros(n, pkg.AAC_STREAM_DT))
    d_rng = torch.full((n,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
    out = dev.aac_parse(cfg, d_st, torch.from_numpy(buf).cuda(), off, coeff_channels=chn)
    dev.spectral_tools(chn, out["coeffs"], out["tools"], rng=d_rng)
    pcm, d_state = dev.lc_decode(chn, out["coeffs"], out["ics"], torch.zeros((n, 512 * chn), device="cuda"), pcm_format=pkg.PCM_F32)
    torch.cuda.synchronize()
    assert not out["status"].cpu().numpy().any()
    assert np.array_equal(out["coeffs"].cpu().numpy().view(np.uint32), ref_c.view(np.uint32))
    assert np.array_equal(pcm.cpu().numpy().view(np.uint32), ref_pcm.view(np.uint32))
    assert np.array_equal(d_state.cpu().numpy().view(np.uint32), ref_state.view(np.uint32))
    assert np.array_equal(d_rng.cpu().numpy(), ref_rng)
    assert np.array_equal(PC.rows(d_st.cpu().numpy(), n), PC.rows(st, n))

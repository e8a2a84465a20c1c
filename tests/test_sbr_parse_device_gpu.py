"""heaac_sbr_parse_device on the GPU against the host parser heaac_heaac_parse_frame_ex: the corpora and the comparison
of test_sbr_core.py through the kernel (one lane per unit) behind heaac_aac_parse_device, state-out and records
pre-filled with 0xA5 on both sides; the combined call heaac_heaac_parse_device; the device-parsed records through
heaac_he_decode_batch; and the call captured into a graph."""
import ctypes as C

import numpy as np
import pytest

import sbr_device_common as SD

pytestmark = pytest.mark.gpu
FILL = SD.FILL


class DeviceChain:
    """n streams: the host's AAC / SBR states and header table as the reference that is carried on, two device state
    arrays that a call ping-pongs between (the rows of deferred units are filled in from the host's parse, as a caller
    does).  One step = heaac_aac_parse_device, heaac_sbr_parse_device on its info and statuses, SD.compare."""

    def __init__(self, pkg, dev, n, cpe):
        import torch
        self.pkg, self.dev, self.n, self.cpe = pkg, dev, n, cpe
        self.cfg = SD.he_cfg(pkg, cpe)
        self.with_ps = not cpe
        self.cc = 2 if cpe else 1
        self.tab = pkg.SbrHeaderTable(256)
        self.st = np.zeros(n, pkg.AAC_STREAM_DT)
        self.sst = pkg.sbr_streams(n)
        self.d_sst = [pkg.to_device(self.sst), torch.empty(self.sst.size, dtype=torch.uint8, device="cuda")]

    def outputs(self):
        import torch
        n, pkg = self.n, self.pkg
        mk = lambda k: torch.full((n * k,), FILL, dtype=torch.uint8, device="cuda")
        return dict(sbr=mk(pkg.SBR_FRAME_DT.itemsize), ps=mk(pkg.PS_FRAME_DT.itemsize) if self.with_ps else None,
                    status=torch.full((n,), 7, dtype=torch.int32, device="cuda"))

    def load(self, aus):
        import torch
        buf, off = self.pkg.pack_units(aus)
        return torch.from_numpy(np.concatenate([buf, np.zeros(4, np.uint8)])).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()

    def records(self, out, d_sst_out):
        import torch
        torch.cuda.synchronize()
        pkg, n = self.pkg, self.n
        return dict(sst=d_sst_out.cpu().numpy().reshape(n, -1), sbr=out["sbr"].cpu().numpy().view(pkg.SBR_FRAME_DT),
                    ps=out["ps"].cpu().numpy().view(pkg.PS_FRAME_DT) if self.with_ps else None, status=out["status"].cpu().numpy())

    def host(self, aus):
        """The host parser from copies of the states: (its records, the AAC states and the SBR states it leaves)."""
        st, sst = self.st.copy(), self.sst.copy()
        return SD.host_parse(self.pkg, self.cfg, st, sst, self.tab, aus, self.cc, self.with_ps), st, sst

    def carry(self, st, sst_host, got_sst, ok):
        """The next call's states: the out rows, with the host's rows for the units it had to take."""
        import torch
        self.st, self.sst = st, sst_host
        self.d_sst.reverse()
        rows = np.flatnonzero(~ok)
        if rows.size:
            d = self.d_sst[0].view(self.n, -1)
            d[torch.from_numpy(rows).cuda()] = torch.from_numpy(sst_host[rows]).cuda()

    def step(self, aus, n_hdr=None, combined=False):
        import torch
        pkg, dev, n = self.pkg, self.dev, self.n
        d_hdr = pkg.to_device(self.tab.headers()[:n_hdr])          # what the device holds: the headers so far
        host, st, sst_host = self.host(aus)
        d_au, d_off = self.load(aus)
        d_st = pkg.to_device(self.st.copy())
        self.d_sst[1].fill_(FILL)
        out = self.outputs()
        if combined:
            res = dev.heaac_parse_device(self.cfg, d_st, self.d_sst[0], d_au, d_off, d_hdr, coeff_channels=self.cc,
                                         sst_out=self.d_sst[1], sbr=out["sbr"], ps=out["ps"], status=out["status"])
        else:
            aac = dev.aac_parse(self.cfg, d_st, d_au, d_off, coeff_channels=self.cc)
            res = dev.sbr_parse_device(self.cfg, self.d_sst[0], d_au, d_off, aac["info"], d_hdr, aac_status=aac["status"],
                                       sst_out=self.d_sst[1], sbr=out["sbr"], ps=out["ps"], status=out["status"])
            res.update(coeffs=aac["coeffs"], ics=aac["ics"], tools=aac["tools"], info=aac["info"], aac_status=aac["status"])
        got = self.records(out, self.d_sst[1])
        assert np.array_equal(self.d_sst[0].cpu().numpy().reshape(n, -1), self.sst), "the in rows were written"
        ok = SD.compare(pkg, host, sst_host, self.sst, got)
        got["dev"] = res
        got["d_st"] = d_st
        self.carry(st, sst_host, got["sst"], ok)
        return host, got, ok


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("cpe", [False, True])
def test_sizes_with_every_class_mixed_in_one_call(pkg, dev, cpe, n):
    """One lane, a wave short by one, a full wave, a block plus one, two blocks plus one; a 4-step chain with ping-ponged
    state.  Behind the streams' first headers every call mixes the classes of SD.CLASSES, so lanes of one wave diverge
    and deferred rows sit beside written ones; one call holds one header fewer than the streams refer to."""
    rng = np.random.default_rng(8100 + 1000 * cpe + n)
    ch = DeviceChain(pkg, dev, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    host, got, ok = ch.step(SD.he_units(rng, writers, cpe))
    assert not host["status"].any() and not ok.any()             # each stream's first header
    in_step = np.ones(n, bool)
    seen = set()
    for step in range(1, 4):
        classes = [SD.CLASSES[int(k)] for k in rng.integers(0, len(SD.CLASSES), n)]
        if n == 1:
            classes = [("plain", "same_header", "new_header")[step - 1]]
        short = step == 2 and len(ch.tab) > 2
        beyond = ch.sst[:, SD.HDR_AT] == len(ch.tab) - 1 if short else np.zeros(n, bool)   # (fewer than 256 headers: one byte)
        host, got, ok = ch.step(SD.mixed_units(rng, writers, cpe, classes), n_hdr=len(ch.tab) - 1 if short else None)
        assert not ok[beyond].any()
        for i, cls in enumerate(classes):
            if cls not in ("flipped", "truncated") and in_step[i] and not beyond[i]:
                assert ok[i] == (cls in ("plain", "same_header", "no_payload")), (step, i, cls, host["status"][i])
                seen.add((cls, bool(ok[i])))
            in_step[i] &= cls not in ("flipped", "truncated", "misplaced", "bad_grid")
    if n >= 63:
        assert {c for c, _ in seen} >= set(SD.CLASSES) - {"flipped", "truncated"}, seen


def test_the_combined_call_equals_the_two_calls_and_the_host(pkg, dev):
    rng = np.random.default_rng(8200)
    n = 65
    for cpe in (False, True):
        two, one = DeviceChain(pkg, dev, n, cpe), DeviceChain(pkg, dev, n, cpe)
        writers = SD.make_writers(pkg, n, cpe)
        for step in range(3):
            if step == 0:
                aus = SD.he_units(rng, writers, cpe)
            else:
                aus = SD.mixed_units(rng, writers, cpe, [SD.CLASSES[int(k)] for k in rng.integers(0, len(SD.CLASSES), n)])
            _, a, ok_a = two.step(aus)
            _, b, ok_b = one.step(aus, combined=True)
            assert np.array_equal(a["status"], b["status"]) and (step == 0 or (ok_a.any() and not ok_a.all()))
            for k in ("sst", "sbr", "ps"):
                if a[k] is not None:
                    assert np.array_equal(a[k][ok_a], b[k][ok_a]), (step, k)
            # the AAC half: the same records, and the same state, as the call by itself leaves
            aac_ok = a["dev"]["aac_status"].cpu().numpy() == 0
            assert aac_ok.sum() > n // 2
            for k in ("coeffs", "ics", "tools", "info"):
                x, y = (r["dev"][k].cpu().numpy().reshape(n, -1).view(np.uint8) for r in (a, b))
                assert np.array_equal(x[aac_ok], y[aac_ok]), (step, k)
            assert np.array_equal(a["d_st"].cpu().numpy(), b["d_st"].cpu().numpy())


@pytest.mark.parametrize("cpe", [False, True])
def test_device_parsed_records_through_the_he_decode(pkg, dev, cpe):
    """64 streams x 3 steady-state steps: bytes -> heaac_heaac_parse_device -> spectral tools -> heaac_he_decode_batch with
    nothing passing through the host, against the same decode fed the host parser's records: PCM and state bit for bit."""
    import torch
    rng = np.random.default_rng(8300 + cpe)
    n = 64
    hcfg = pkg.CFG_HEV1 if cpe else pkg.CFG_HEV2
    chn = 2 if cpe else 1
    ch = DeviceChain(pkg, dev, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    ch.step(SD.he_units(rng, writers, cpe))                       # the first headers: the host's
    d_hdr = pkg.to_device(ch.tab.headers())
    state = [torch.zeros((n, pkg.STATE_WORDS[hcfg]), device="cuda") for _ in range(2)]
    rngs = [torch.full((n,), 0x1f2e3d4c, dtype=torch.int32, device="cuda") for _ in range(2)]
    for step in range(3):
        aus = SD.he_units(rng, writers, cpe)
        host, got, ok = ch.step(aus, combined=True)
        assert not host["status"].any() and ok.all()
        d = got["dev"]
        pcm = []
        for side in range(2):
            if side == 0:
                coeffs, ics, tools, sbr, ps = d["coeffs"].clone(), d["ics"], d["tools"], d["sbr"], d["ps"]
            else:
                coeffs, ics, tools = d["coeffs"].clone(), d["ics"], d["tools"]     # (the AAC half has its own tests)
                sbr, ps = pkg.to_device(host["sbr"]), pkg.to_device(host["ps"]) if not cpe else None
            dev.spectral_tools(chn, coeffs, tools, rng=rngs[side])
            # the writer's escape values reach far beyond full scale: bring the spectrum down by a power of two
            peak = coeffs.abs().amax(dim=(1, 2)).clamp(min=1.0)
            coeffs.mul_(torch.exp2(-torch.ceil(torch.log2(peak)))[:, None, None])
            assert dev.he_check(hcfg, sbr, d_hdr, ps) is None
            p, state[side] = dev.he_decode(hcfg, coeffs, ics, sbr, d_hdr, ps, state[side])
            pcm.append(p.cpu().numpy())
        assert np.array_equal(pcm[0].view(np.uint32), pcm[1].view(np.uint32)), step
        assert np.array_equal(state[0].cpu().numpy().view(np.uint32), state[1].cpu().numpy().view(np.uint32)), step
        assert np.isfinite(pcm[0]).all() and np.abs(pcm[0]).max() > 0, step


def test_captured_into_a_graph_and_replayed(pkg, dev):
    """heaac_sbr_parse_device captured once on a side stream and replayed twice on 0xA5-refilled outputs: the same bytes
    each time, and the bytes the contract asks for."""
    import torch
    rng = np.random.default_rng(8400)
    n, cpe = 129, False
    ch = DeviceChain(pkg, dev, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    ch.step(SD.he_units(rng, writers, cpe))
    aus = SD.mixed_units(rng, writers, cpe, [SD.CLASSES[int(k)] for k in rng.integers(0, len(SD.CLASSES), n)])
    host, _, sst_host = ch.host(aus)
    d_hdr = pkg.to_device(ch.tab.headers())
    d_au, d_off = ch.load(aus)
    aac = dev.aac_parse(ch.cfg, pkg.to_device(ch.st.copy()), d_au, d_off, coeff_channels=1)
    out = ch.outputs()
    d_in, d_out = ch.d_sst

    def refill():
        d_out.fill_(FILL)
        out["sbr"].fill_(FILL)
        out["ps"].fill_(FILL)
        out["status"].fill_(7)

    def call():
        dev.sbr_parse_device(ch.cfg, d_in, d_au, d_off, aac["info"], d_hdr, aac_status=aac["status"], sst_out=d_out,
                             sbr=out["sbr"], ps=out["ps"], status=out["status"])

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()                                         # warm-up on the capture stream
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    seen = []
    for _ in range(2):
        refill()
        torch.cuda.synchronize()
        g.replay()
        got = ch.records(out, d_out)
        ok = SD.compare(pkg, host, sst_host, ch.sst, got)
        assert ok.any() and not ok.all()
        seen.append(got)
    for k in ("sst", "sbr", "ps", "status"):
        assert np.array_equal(seen[0][k], seen[1][k]), k


def test_device_entry_refuses_bad_arguments_before_any_launch(pkg, dev):
    """heaac_sbr_parse_device itself, with a real device: every array NULL in turn, state arrays that are the same or
    overlap, n_hdr = 0, a mono PS configuration without d_ps, a misaligned record array and an n beyond the grid are
    HEAAC_ERR_ARG and write nothing; n = 0 is HEAAC_OK whatever the arrays are."""
    import torch
    f = pkg.lib().heaac_sbr_parse_device
    rng = np.random.default_rng(8500)
    n = 4
    ch = DeviceChain(pkg, dev, n, False)
    writers = SD.make_writers(pkg, n, False)
    ch.step(SD.he_units(rng, writers, False))
    aus = SD.he_units(rng, writers, False)
    d_au, d_off = ch.load(aus)
    aac = dev.aac_parse(ch.cfg, pkg.to_device(ch.st.copy()), d_au, d_off, coeff_channels=1)
    d_hdr = pkg.to_device(ch.tab.headers())
    out = ch.outputs()
    d_in, d_out = ch.d_sst
    d_out.fill_(FILL)
    three = torch.zeros(3 * ch.sst.shape[1], dtype=torch.uint8, device="cuda")
    row = ch.sst.shape[1]
    good = [dev._h, C.addressof(ch.cfg), d_in.data_ptr(), d_out.data_ptr(), d_au.data_ptr(), d_off.data_ptr(),
            aac["info"].data_ptr(), aac["status"].data_ptr(), n, d_hdr.data_ptr(), len(ch.tab), out["sbr"].data_ptr(),
            out["ps"].data_ptr(), out["status"].data_ptr(), None]

    def untouched():
        torch.cuda.synchronize()
        assert (out["status"].cpu().numpy() == 7).all()
        for t in (d_out, out["sbr"], out["ps"]):
            assert (t.cpu().numpy() == FILL).all()

    for k in (0, 1, 2, 3, 4, 5, 6, 9, 11, 12, 13):
        bad = list(good)
        bad[k] = None
        assert f(*bad) == -1, k
    for a, b in ((d_in.data_ptr(), d_in.data_ptr()), (three.data_ptr(), three.data_ptr() + row), (three.data_ptr() + row, three.data_ptr())):
        bad = list(good)
        bad[2], bad[3], bad[8] = a, b, 2
        assert f(*bad) == -1
    for k, v in ((10, 0), (11, out["sbr"].data_ptr() + 2), (8, 0x7fffffff * 64 + 1)):
        bad = list(good)
        bad[k] = v
        assert f(*bad) == -1, k
    untouched()
    zero = list(good)
    zero[8] = 0
    assert f(*zero) == 0
    for k in (2, 3, 4, 5, 6, 7, 9, 11, 12, 13):
        zero[k] = None
    zero[10] = 0
    assert f(*zero) == 0
    untouched()
    assert f(*good) == 0                                  # and the same arguments as they should be parse
    torch.cuda.synchronize()
    assert not out["status"].cpu().numpy().any()

"""The prep kernel of the device parsers (k_parse_prep: records zeroed, SBR state rows copied in -> out) on arrays that
are 4-byte but not 16-byte aligned.  Torch allocations are 256-byte aligned, so no other test reaches the head path of
the zero fill, the head / body / tail split of the 16-byte copy or the 4-byte copy it falls back to when the two state
arrays do not share their alignment.

Each call runs once on fresh, aligned tensors as the reference.  Then every array the prep kernel fills or copies
(tools, sbr, ps, sst_out) is the slice [off : off + len] of a uint8 tensor of len + 32 bytes of 0xA5, for off = 4, 8
and 12; sst_in once at the same offset as sst_out (16-byte words with a head and a tail) and once at (off + 8) % 16
(4-byte words).  Every output equals the reference byte for byte, and the off bytes in front of each slice and the
32 - off bytes behind it are still 0xA5: at these sizes a wrong head, body or tail count writes out of the slice or
leaves a word of it unzeroed."""
import numpy as np
import pytest

import parse_device_common as PC
import parse_streams_common as PS
import sbr_device_common as SD
import test_parse as TP
import test_parse_streams_gpu as TSG
import test_sbr_parse_device_gpu as TSB

pytestmark = pytest.mark.gpu
FILL = PC.FILL
PAD = 32
OFFSETS = (4, 8, 12)


def fresh(nbytes, dtype=None):
    """An aligned output tensor of nbytes bytes of FILL."""
    import torch
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    return t if dtype is None else t.view(dtype)


class Carved:
    """Arrays as slices [off : off + len] of FILLed tensors of len + PAD bytes."""

    def __init__(self):
        self.bases = []

    def __call__(self, nbytes, off, src=None):
        import torch
        base = torch.full((nbytes + PAD,), FILL, dtype=torch.uint8, device="cuda")
        assert base.data_ptr() % 16 == 0
        part = base[off:off + nbytes]
        if src is not None:
            part.copy_(src.reshape(-1))
        self.bases.append((base, off, nbytes))
        return part

    def guards_intact(self):
        for base, off, nbytes in self.bases:
            b = base.cpu().numpy()
            assert (b[:off] == FILL).all() and (b[off + nbytes:] == FILL).all(), (off, nbytes)


def against_aligned(call, with_state):
    """call(carve, off, in_off) -> dict of every output tensor, the arrays of the prep kernel made by carve(nbytes, off)
    and sst_in by carve(nbytes, in_off, src)."""
    import torch

    def run(off, in_off):
        carve = Carved()
        out = call(carve, off, in_off)
        torch.cuda.synchronize()
        carve.guards_intact()
        return {k: v.cpu().numpy().reshape(-1).view(np.uint8) for k, v in out.items() if v is not None}

    ref = run(0, 0)
    for off in OFFSETS:
        for in_off in ((off, (off + 8) % 16) if with_state else (off,)):
            got = run(off, in_off)
            assert got.keys() == ref.keys()
            for k in ref:
                assert np.array_equal(got[k], ref[k]), (off, in_off, k, np.flatnonzero(got[k] != ref[k])[:8])
    return ref


@pytest.mark.parametrize("n", [1, 2, 5])
def test_aac_parse_on_misaligned_tools(pkg, dev, n):
    import torch
    rng = np.random.default_rng(1700 + n)
    cfg = TP._cfg(pkg, 2, 3, 2)
    aus = PC.in_scope_steps(rng, 3, 2, True, n, 1, adts=0.3, sbr=0.3)[0]
    d_au, d_off = TSG.load(pkg, aus)

    def call(carve, off, in_off):
        d_st = torch.zeros(n * pkg.AAC_STREAM_DT.itemsize, dtype=torch.uint8, device="cuda")
        out = dev.aac_parse(cfg, d_st, d_au, d_off, coeff_channels=2, coeffs=fresh(n * 2 * 1024 * 4, torch.float32),
                            ics=fresh(n * 2 * pkg.ICS_DT.itemsize), tools=carve(n * pkg.TOOLS_FRAME_DT.itemsize, off),
                            info=fresh(n * pkg.AAC_INFO_DT.itemsize), status=fresh(n * 4, torch.int32))
        return dict(out, st=d_st)

    ref = against_aligned(call, False)
    assert not ref["status"].any()


@pytest.mark.parametrize("n", [1, 2, 5])
def test_sbr_parse_device_on_misaligned_state_rows_and_records(pkg, dev, n):
    import torch
    rng = np.random.default_rng(1710 + n)
    ch = TSB.DeviceChain(pkg, dev, n, False)                  # mono with Parametric Stereo
    writers = SD.make_writers(pkg, n, False)
    ch.step(SD.he_units(rng, writers, False))                 # the first headers: the host's
    d_au, d_off = ch.load(SD.he_units(rng, writers, False))
    aac = dev.aac_parse(ch.cfg, pkg.to_device(ch.st.copy()), d_au, d_off, coeff_channels=1)
    d_hdr = pkg.to_device(ch.tab.headers())
    d_in = ch.d_sst[0]

    def call(carve, off, in_off):
        sst_in = carve(d_in.numel(), in_off, d_in)
        out = dev.sbr_parse_device(ch.cfg, sst_in, d_au, d_off, aac["info"], d_hdr, aac_status=aac["status"],
                                   sst_out=carve(d_in.numel(), off), sbr=carve(n * pkg.SBR_FRAME_DT.itemsize, off),
                                   ps=carve(n * pkg.PS_FRAME_DT.itemsize, off), status=fresh(n * 4, torch.int32))
        return dict(out, sst_in=sst_in)

    ref = against_aligned(call, True)
    assert not ref["status"].any() and (ref["ps"] != FILL).any()
    assert np.array_equal(ref["sst_in"].reshape(n, -1), ch.sst), "the in rows were written"


@pytest.mark.parametrize("S,T", [(1, 1), (2, 3)])
def test_heaac_parse_device_streams_on_misaligned_state_rows_and_records(pkg, dev, S, T):
    import torch
    rng = np.random.default_rng(1720 + S)
    h = TSG.HeStreams(pkg, rng, S, False, "20")               # mono with Parametric Stereo
    d_au, d_off = TSG.load(pkg, PS.flat([SD.he_units(rng, h.writers, False) for _ in range(T)]))
    d_hdr = pkg.to_device(h.tab.headers())
    d_in = pkg.to_device(h.sst)
    n = S * T

    def call(carve, off, in_off):
        d_st = pkg.to_device(h.st.copy())
        sst_in = carve(d_in.numel(), in_off, d_in)
        out = dev.heaac_parse_device_streams(h.cfg, d_st, sst_in, d_au, d_off, d_hdr, T, coeff_channels=1,
                                             coeffs=fresh(n * 1024 * 4, torch.float32), ics=fresh(n * pkg.ICS_DT.itemsize),
                                             tools=carve(n * pkg.TOOLS_FRAME_DT.itemsize, off), info=fresh(n * pkg.AAC_INFO_DT.itemsize),
                                             sst_out=carve(d_in.numel(), off), sbr=carve(n * pkg.SBR_FRAME_DT.itemsize, off),
                                             ps=carve(n * pkg.PS_FRAME_DT.itemsize, off), status=fresh(n * 4, torch.int32),
                                             taken=fresh(S * 4, torch.int32), hold=fresh(n))
        return dict(out, st=d_st, sst_in=sst_in)

    ref = against_aligned(call, True)
    assert not ref["status"].any() and (ref["taken"].view(np.uint32) == T).all() and (ref["ps"] != FILL).any()
    assert np.array_equal(ref["sst_in"].reshape(S, -1), h.sst), "the in rows were written"

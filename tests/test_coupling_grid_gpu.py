"""The multichannel back end on the GPU over the records of tests/edge_coupling.py (tests/test_coupling_reach.py holds
what they reach, as exact sets, and pins the oracle's coupling to an independent restatement):

  tools_dependent_coupling in k_spectral_tools   heaac_spectral_tools_batch_ex with HeaacCceFrame records: every
      profile x mono / stereo targets x TOOLS_ALL, TOOLS_PRE then TOOLS_POST, TOOLS_POST alone; batches of 1, 9, 10
      and 11 frames (a workgroup is 10 waves), the whole profile, and 2 571 frames (a wave takes a second frame)
  k_couple                                       heaac_couple_after_imdct_batch: all `on` patterns, with and without
      the int16 output, three chained calls, every golden gain, sums at both int16 limits, the codec's channels = 1
      form over a 2048-sample plane
  k_interleave, k_interleave_packed<fmt, 1 .. 8> heaac_pcm_interleave_batch: every channel count x both formats x
      len 4 / 12 / 1024 / 2048 x n 1 / 2 / 65 x an 8-byte aligned output and one displaced by one int16 (where
      1 .. 8 channels take k_interleave too), on the edges of both conversions

Against the oracle, bit for bit: float words as uint32 (a NaN matched by any NaN), generator words and int16 equal."""
import ctypes as C

import numpy as np
import pytest

import edge_coupling as K

pytestmark = pytest.mark.gpu


def _assert_words(got, ref, what):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ok = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert ok.all(), "%s: %d words differ, first at %s" % (what, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _tools_call(pkg, dev, channels, form, d_c, d_t, d_r, d_cce, d_cc):
    if form == "all":
        dev.spectral_tools_ex(channels, pkg.TOOLS_ALL, d_c, d_t, rng=d_r, cce=d_cce, cce_coeffs=d_cc)
    elif form == "pre_post":
        dev.spectral_tools_ex(channels, pkg.TOOLS_PRE, d_c, d_t, rng=d_r)
        dev.spectral_tools_ex(channels, pkg.TOOLS_POST, d_c, d_t, cce=d_cce, cce_coeffs=d_cc)
    else:
        dev.spectral_tools_ex(channels, pkg.TOOLS_POST, d_c, d_t, rng=d_r, cce=d_cce, cce_coeffs=d_cc)


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", K.PROFILES)
def test_dependent_coupling(pkg, oracle, dev, profile, channels, form):
    """the target spectrum and the generator word are the oracle's, the coupling channels' spectra are left alone,
    and the NaN gains and spectra the records hide are never read (the result holds no NaN)"""
    u = K.units(pkg, profile, channels)
    ref_c, ref_r = K.oracle_run(pkg, oracle, profile, channels, form)
    n = len(u["tools"])
    for count in sorted({1, 9, 10, 11, n}):
        assert count <= n
        d_c, d_r, d_cc = _cuda(u["coeffs"][:count]), _cuda(u["rng"][:count]), _cuda(u["cce_coeffs"][:count])
        _tools_call(pkg, dev, channels, form, d_c, pkg.to_device(np.array(u["tools"][:count])), d_r,
                    pkg.to_device(np.array(u["cce"][:count])), d_cc)
        what = "%d frames" % count
        got = d_c.cpu().numpy()
        _assert_words(got, ref_c[:count], what + ", coefficients")
        assert np.array_equal(d_r.cpu().numpy(), ref_r[:count]), what + ", generator"
        assert np.array_equal(d_cc.cpu().numpy().view(np.uint32), u["cce_coeffs"][:count].view(np.uint32)), what
        assert not np.isnan(got).any(), what


@pytest.mark.parametrize("channels", [1, 2])
def test_dependent_coupling_position_independent(pkg, oracle, dev, channels):
    """2 571 frames, one more than 256 workgroups x 10 waves, with two coupling slots: a 64-frame oracle-checked set
    (`tables`) tiled across the batch; every tile reproduces the oracle wherever in the grid it lands"""
    import torch
    u = K.units(pkg, "tables", channels)
    ref_c, ref_r = K.oracle_run(pkg, oracle, "tables", channels, "all")
    base, n = 64, 2571
    reps = -(-n // base)
    tile = lambda t: t.repeat((reps,) + (1,) * (t.dim() - 1))[:n].contiguous()
    d_c, d_r, d_cc = (tile(_cuda(u[k][:base])) for k in ("coeffs", "rng", "cce_coeffs"))
    d_t = pkg.to_device(np.array(u["tools"][:base])).repeat(reps)[: n * pkg.TOOLS_FRAME_DT.itemsize].contiguous()
    d_cce = pkg.to_device(np.array(u["cce"][:base])).repeat(reps)[: n * 2 * pkg.CCE_FRAME_DT.itemsize].contiguous()
    _tools_call(pkg, dev, channels, "all", d_c, d_t, d_r, d_cce, d_cc)
    want_c, want_r = tile(_cuda(ref_c[:base])), tile(_cuda(ref_r[:base]))
    assert not bool(torch.isnan(want_c).any())
    assert bool((d_c.view(torch.int32) == want_c.view(torch.int32)).all())
    assert bool((d_r == want_r).all())
    assert bool((d_cc.view(torch.int32) == tile(_cuda(u["cce_coeffs"][:base])).view(torch.int32)).all())


# ---------------------------------------------------------------------------
# k_couple
# ---------------------------------------------------------------------------
def _couple_chain(pkg, oracle, dev, channels, pcm, steps, s16, what):
    ref, d_pcm = pcm, _cuda(pcm)
    for k, (cce, cpl) in enumerate(steps):
        ref, r16 = oracle.couple_after_imdct_batch(channels, ref, cce, cpl, s16=s16)
        d_cce = _cuda(cce)
        g16 = dev.couple_after_imdct(channels, d_pcm, d_cce, pkg.to_device(cpl), s16=s16)
        _assert_words(d_pcm.cpu().numpy(), ref, "%s call %d" % (what, k))
        assert np.array_equal(d_cce.cpu().numpy().view(np.uint32), cce.view(np.uint32)), (what, k)
        assert (g16 is None) == (not s16)
        if s16:
            assert np.array_equal(g16.cpu().numpy(), r16), (what, k, np.argwhere(g16.cpu().numpy() != r16)[:4])
    return ref


@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("on", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_couple_after_imdct(pkg, oracle, dev, on, channels, s16):
    """three chained calls for n = 1, 2 and 257; an uncoupled channel's gain is NaN and its samples keep their words;
    frame 0 of the first call lands on, one step inside and one step outside both int16 limits"""
    for n in (1, 2, 257):
        pcm, steps = K.couple_case(pkg, n, channels, on)
        ref = _couple_chain(pkg, oracle, dev, channels, pcm, steps, s16, "n %d" % n)
        assert not np.isnan(ref).any()
        for c in range(channels):
            if not on[c]:
                assert np.array_equal(ref[:, c].view(np.uint32), pcm[:, c].view(np.uint32))


def test_couple_every_golden_gain(pkg, oracle, dev):
    pcm, steps = K.couple_golden(pkg)
    ref = _couple_chain(pkg, oracle, dev, 2, pcm, steps, True, "golden")
    assert np.isinf(ref).any() and not np.isnan(ref).any()


def test_couple_a_2048_sample_plane_as_two_rows(pkg, oracle, dev):
    """the codec's form behind SBR: channels = 1, one 2048-sample plane per frame as two rows of 1024 with one
    HeaacCoupling each (the same gain), the coupling channel's 2048 samples likewise"""
    frames = 3
    pcm, steps = K.couple_case(pkg, 2 * frames, 1, (1, 1), calls=2, seed=1)
    for cce, cpl in steps:
        cpl["gain"][1::2] = cpl["gain"][0::2]
    plane = pcm.reshape(frames, 2048)
    ref = _couple_chain(pkg, oracle, dev, 1, plane.reshape(2 * frames, 1, 1024), steps, False, "2048")
    want = plane.copy()
    for cce, cpl in steps:
        want = want + np.repeat(cpl["gain"][0::2, 0], 2048).reshape(frames, 2048) * (cce.reshape(frames, 2048) - K.BIAS)
    _assert_words(ref.reshape(frames, 2048), want, "a plane at once")


# ---------------------------------------------------------------------------
# interleave
# ---------------------------------------------------------------------------
GUARD = 0x5a5a


def _interleave(pkg, dev, pool, planes, length, n, fmt, displaced):
    """heaac_pcm_interleave_batch into a guarded buffer, the output 8-byte aligned or displaced by one int16"""
    import torch
    ch = len(planes)
    words = n * length * ch
    out = torch.full((words + 1 + 8,), GUARD, dtype=torch.int16, device="cuda")
    assert out.data_ptr() % 8 == 0 and pool.data_ptr() % 16 == 0
    refs = (pkg._PlaneRef * ch)()
    for c, (off, stride) in enumerate(planes):
        refs[c].d_base = pool.data_ptr() + 4 * off
        refs[c].frame_stride = stride
    first = 1 if displaced else 0
    rc = pkg.lib().heaac_pcm_interleave_batch(dev._h, ch, refs, int(length), int(fmt),
                                              C.c_void_p(out.data_ptr() + 2 * first), C.c_size_t(n), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:first] == GUARD).all() and (got[first + words:] == GUARD).all(), "wrote outside its output"
    return got[first: first + words].reshape(n, length, ch)


@pytest.mark.parametrize("channels", range(1, 17))
@pytest.mark.parametrize("sse2", [False, True])
def test_interleave_every_channel_count(pkg, oracle, dev, channels, sse2):
    """len 4 / 12 / 1024 / 2048 x n 1 / 2 / 65 x aligned / displaced output; planes in pair buffers, at wide strides,
    named twice and with frame_stride 0, over the edges of the conversion"""
    fmt = pkg.PCM_S16_SSE2 if sse2 else pkg.PCM_S16
    for length in (4, 12, 1024, 2048):
        for n in (1, 2, 65):
            planes, size = K.interleave_planes(channels, length, n)
            host = K.interleave_pool(sse2, size)
            pool = _cuda(host)
            want = np.stack([oracle.float_to_int16_interleave([host[o + f * s: o + f * s + length] for o, s in planes],
                                                              sse2=sse2) for f in range(n)])
            for displaced in (False, True):
                got = _interleave(pkg, dev, pool, planes, length, n, fmt, displaced)
                assert np.array_equal(got, want), (length, n, displaced, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("channels,displaced", [(1, False), (1, True), (5, False), (5, True), (7, False), (12, False)])
def test_interleave_every_c_path_float(pkg, oracle, dev, channels, displaced):
    """all 65 536 floats 385 + k / 32768 give k, in every channel (each plane starts at another k); the floats next
    beyond either end and far beyond clip, +-inf and NaN are what the oracle makes of their bits"""
    vals = K.c_path_values()
    edges = K.interleave_edges(False)
    host = np.concatenate([vals, vals, edges, np.full((-len(edges)) % 4, 385.0, np.float32)])
    pool = _cuda(host)
    planes = [(4096 * c, 0) for c in range(channels)]
    got = _interleave(pkg, dev, pool, planes, 65536, 1, pkg.PCM_S16, displaced)[0]
    k = np.arange(-32768, 32768)
    for c in range(channels):
        want = (k + 4096 * c + 32768) % 65536 - 32768
        assert np.array_equal(got[:, c].astype(np.int64), want), c
    edges = host[2 * 65536:]
    assert len(edges) % 4 == 0
    got = _interleave(pkg, dev, pool, [(2 * 65536, 0)] * channels, len(edges), 1, pkg.PCM_S16, displaced)[0]
    want = oracle.float_to_int16_interleave([edges] * channels)
    assert np.array_equal(got, want)
    assert got[0, 0] == 32767 and got[1, 0] == -32768

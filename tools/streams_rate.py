"""The streams form (heaac_he_decode_streams / heaac_lc_decode_streams: S streams x T consecutive frames, state in once
and out once per stream) against the batch form (heaac_he_decode_batch_ex / heaac_lc_decode_batch: every frame an
independent unit with its own state record in and out) on the same 262 144 frames.  A and B alternate, each timed with HIP events on the launch stream; the best of
`reps` is kept.  roofline.frac uses the same algorithmic bytes per frame as bench.py for both forms (85 284 for
HE-AACv2, 83 976 for HE-AACv1, 24 584 / 12 292 / 20 488 for AAC-LC stereo / mono / stereo int16: SURVEY s8d -- never a
smaller denominator for the streams form).
The spectral tools (heaac_spectral_tools_streams against heaac_spectral_tools_batch with per-frame generator and
predictor records) use tools/tools_rate.py's bytes per frame for both forms: 23 516 for tools_lc_stereo (noise
substitution on), 88 028 / 44 080 for tools_main_stereo / tools_main_mono (noise substitution and AAC-Main prediction).
One JSON line per (workload, T).
usage: python tools/streams_rate.py [--frames 262144] [--reps 5] [--warmup 1] [--T 1,2,4,8]
                                    [--workloads hev2,hev2_s16,hev1,lc_stereo,lc_mono,lc_stereo_s16,
                                                 tools_lc_stereo,tools_main_stereo,tools_main_mono]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as G

pkg = G.load_package()
synth = importlib.import_module("ffmpeg_heaac_amd.synth")

WORKLOADS = {"hev2": ("CFG_HEV2", "PCM_F32"), "hev2_s16": ("CFG_HEV2", "PCM_S16"), "hev1": ("CFG_HEV1", "PCM_F32")}
# AAC-LC: channels, PCM format (the batch form's algorithmic bytes per frame: coefficients, overlap in and out, PCM, ICS)
LC_WORKLOADS = {"lc_stereo": (2, "PCM_F32"), "lc_mono": (1, "PCM_F32"), "lc_stereo_s16": (2, "PCM_S16")}
# spectral tools: channels, AAC-Main prediction (noise substitution is on in all three)
TOOLS_WORKLOADS = {"tools_lc_stereo": (2, False), "tools_main_stereo": (2, True), "tools_main_mono": (1, True)}


def lc_bytes_per_frame(channels, fmt):
    return channels * (4096 + 2048 + 2048 + (4096 if fmt == pkg.PCM_F32 else 2048) + 4)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed A, B calls before the timed reps")
    ap.add_argument("--T", default="1,2,4,8")
    ap.add_argument("--workloads", default="hev2,hev2_s16,hev1")
    ap.add_argument("--pool", type=int, default=1024, help="distinct streams generated; the rest are copies")
    a = ap.parse_args()
    n = a.frames
    dev = pkg.Device(n)
    hdr = synth.default_headers(pkg)
    d_hdr = pkg.to_device(hdr)
    Ts = [int(x) for x in a.T.split(",")]
    for wl in a.workloads.split(","):
        if wl in LC_WORKLOADS:
            run_lc(a, dev, wl, Ts)
            continue
        if wl in TOOLS_WORKLOADS:
            run_tools(a, dev, wl, Ts)
            continue
        cfg_name, fmt_name = WORKLOADS[wl]
        cfg, fmt = getattr(pkg, cfg_name), getattr(pkg, fmt_name)
        words, nout = pkg.STATE_WORDS[cfg], pkg.OUT_CH[cfg]
        rng = np.random.default_rng(5)
        frs = list(synth.he_stream(rng, cfg, a.pool, max(Ts), hdr, ps_mode="20"))
        pcm = (torch.empty((n, nout, 2048), device="cuda") if fmt == pkg.PCM_F32
               else torch.empty((n, 2048, nout), dtype=torch.int16, device="cuda"))
        for T in Ts:
            S = n // T
            assert S * T == n and S % a.pool == 0
            # [pool][T] frames, stream s = pool stream s % pool; frame (s, t) at s * T + t
            def stack(k):
                x = np.stack([f[k] for f in frs[:T]], axis=1)
                x = np.tile(x, (S // a.pool,) + (1,) * (x.ndim - 1))
                return np.ascontiguousarray(x.reshape((n,) + x.shape[2:]))
            coeffs = torch.from_numpy(stack("coeffs")).cuda()
            ics, sbr = pkg.to_device(stack("ics")), pkg.to_device(stack("sbr"))
            ps = pkg.to_device(stack("ps")) if cfg == pkg.CFG_HEV2 else None
            st_s = torch.zeros((S, words), device="cuda")
            st_s2 = torch.empty_like(st_s)
            st_b = torch.zeros((n, words), device="cuda")
            st_b2 = torch.empty_like(st_b)
            run_a = lambda: dev.he_decode_streams(cfg, coeffs, ics, sbr, d_hdr, ps, st_s, T, state_out=st_s2, pcm=pcm,
                                                  pcm_format=fmt)
            run_b = lambda: dev.he_decode(cfg, coeffs, ics, sbr, d_hdr, ps, st_b, state_out=st_b2, pcm=pcm, pcm_format=fmt)
            for _ in range(a.warmup):
                run_a(); run_b()
            ta, tb = [], []
            for _ in range(a.reps):
                ta.append(timed(run_a))
                tb.append(timed(run_b))
            ms_a, ms_b = min(ta), min(tb)
            bpf = pkg.ALGO_BYTES[cfg] - (nout * 2048 * 2 if fmt != pkg.PCM_F32 else 0)
            rec = dict(workload=wl, T=T, streams=S, frames=n, streams_ms=round(ms_a, 4), batch_ms=round(ms_b, 4),
                       speedup=round(ms_b / ms_a, 4), streams_frames_per_s=round(n / (ms_a * 1e-3)),
                       batch_frames_per_s=round(n / (ms_b * 1e-3)), bytes_per_frame=bpf,
                       roofline={"frac": round(bpf * n / (ms_a * 1e-3) / 8e12, 4),
                                 "batch_frac": round(bpf * n / (ms_b * 1e-3) / 8e12, 4)},
                       samples_ms={"streams": [round(x, 4) for x in ta], "batch": [round(x, 4) for x in tb]})
            print(json.dumps(rec), flush=True)
            del coeffs, ics, sbr, ps, st_s, st_s2, st_b, st_b2
            torch.cuda.empty_cache()
    dev.close()


def run_lc(a, dev, wl, Ts):
    n = a.frames
    channels, fmt_name = LC_WORKLOADS[wl]
    fmt = getattr(pkg, fmt_name)
    bpf = lc_bytes_per_frame(channels, fmt)
    assert channels != 2 or bpf == pkg.ALGO_BYTES[pkg.CFG_LC_STEREO] - (2048 * 2 if fmt != pkg.PCM_F32 else 0)
    rng = np.random.default_rng(5)
    steps = list(synth.lc_stream(rng, a.pool, max(Ts), channels))
    pcm = (torch.empty((n, channels, 1024), device="cuda") if fmt == pkg.PCM_F32
           else torch.empty((n, 1024, channels), dtype=torch.int16, device="cuda"))
    for T in Ts:
        S = n // T
        assert S * T == n and S % a.pool == 0
        # [pool][T] frames, stream s = pool stream s % pool; frame (s, t) at s * T + t
        def stack(k):
            x = np.stack([st[k] for st in steps[:T]], axis=1)
            x = np.tile(x, (S // a.pool,) + (1,) * (x.ndim - 1))
            return np.ascontiguousarray(x.reshape((n,) + x.shape[2:]))
        coeffs, ics = torch.from_numpy(stack(0)).cuda(), pkg.to_device(stack(1))
        st_s = torch.zeros((S, channels * 512), device="cuda")
        st_s2 = torch.empty_like(st_s)
        st_b = torch.zeros((n, channels * 512), device="cuda")
        st_b2 = torch.empty_like(st_b)
        run_a = lambda: dev.lc_decode_streams(channels, coeffs, ics, st_s, T, state_out=st_s2, pcm=pcm, pcm_format=fmt)
        run_b = lambda: dev.lc_decode(channels, coeffs, ics, st_b, state_out=st_b2, pcm=pcm, pcm_format=fmt)
        for _ in range(a.warmup):
            run_a(); run_b()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timed(run_a))
            tb.append(timed(run_b))
        ms_a, ms_b = min(ta), min(tb)
        rec = dict(workload=wl, T=T, streams=S, frames=n, streams_ms=round(ms_a, 4), batch_ms=round(ms_b, 4),
                   speedup=round(ms_b / ms_a, 4), streams_frames_per_s=round(n / (ms_a * 1e-3)),
                   batch_frames_per_s=round(n / (ms_b * 1e-3)), bytes_per_frame=bpf,
                   roofline={"frac": round(bpf * n / (ms_a * 1e-3) / 8e12, 4),
                             "batch_frac": round(bpf * n / (ms_b * 1e-3) / 8e12, 4)},
                   samples_ms={"streams": [round(x, 4) for x in ta], "batch": [round(x, 4) for x in tb]})
        print(json.dumps(rec), flush=True)
        del coeffs, ics, st_s, st_s2, st_b, st_b2
        torch.cuda.empty_cache()


def tools_bytes_per_frame(channels, main):
    """tools/tools_rate.py's count: coefficients in and out, the record, the predictors in and out"""
    return channels * 8192 + (pkg.TOOLS_FRAME_DT.itemsize if channels == 2 else 132 + 3500) + \
        (channels * pkg.MAX_PREDICTORS * 24 * 2 if main else 0)


def run_tools(a, dev, wl, Ts):
    n = a.frames
    channels, main = TOOLS_WORKLOADS[wl]
    bpf = tools_bytes_per_frame(channels, main)
    rng = np.random.default_rng(5)
    # [pool][max T] records and spectra; stream s = pool stream s % pool
    tf = np.stack([synth.tools_frames(rng, pkg, a.pool, channels) for _ in range(max(Ts))], axis=1)
    cf = (rng.standard_normal((a.pool, max(Ts), channels, 1024)) * 1e-4).astype(np.float32)
    pred0 = torch.tensor([0, 0, 1, 1, 0, 0], dtype=torch.float32, device="cuda")   # reset_all_predictors
    for T in Ts:
        S = n // T
        assert S * T == n and S % a.pool == 0
        def stack(x):
            x = np.tile(x[:, :T], (S // a.pool,) + (1,) * (x.ndim - 1))
            return np.ascontiguousarray(x.reshape((n,) + x.shape[2:]))
        coeffs0 = torch.from_numpy(stack(cf)).cuda()
        coeffs = torch.empty_like(coeffs0)
        tools = pkg.to_device(stack(tf))
        rng_s = torch.full((S,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
        rng_b = torch.full((n,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
        pred_s = pred0.repeat(S * channels * pkg.MAX_PREDICTORS).view(S, channels, pkg.MAX_PREDICTORS, 6) if main else None
        pred_b = pred0.repeat(n * channels * pkg.MAX_PREDICTORS).view(n, channels, pkg.MAX_PREDICTORS, 6) if main else None
        run_a = lambda: dev.spectral_tools_streams(channels, coeffs, tools, T, rng=rng_s, pred=pred_s)
        run_b = lambda: dev.spectral_tools(channels, coeffs, tools, rng=rng_b, pred=pred_b)

        def fresh(fn):                       # every call on the same spectra (outside the timed region)
            coeffs.copy_(coeffs0)
            return timed(fn)
        for _ in range(a.warmup):
            fresh(run_a); fresh(run_b)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(fresh(run_a))
            tb.append(fresh(run_b))
        ms_a, ms_b = min(ta), min(tb)
        rec = dict(workload=wl, T=T, streams=S, frames=n, streams_ms=round(ms_a, 4), batch_ms=round(ms_b, 4),
                   speedup=round(ms_b / ms_a, 4), streams_frames_per_s=round(n / (ms_a * 1e-3)),
                   batch_frames_per_s=round(n / (ms_b * 1e-3)), bytes_per_frame=bpf,
                   streams_bytes_per_frame_projected=round(bpf - (channels * pkg.MAX_PREDICTORS * 24 * 2 * (1 - 1 / T)
                                                                  if main else 0), 1),
                   roofline={"frac": round(bpf * n / (ms_a * 1e-3) / 8e12, 4),
                             "batch_frac": round(bpf * n / (ms_b * 1e-3) / 8e12, 4)},
                   samples_ms={"streams": [round(x, 4) for x in ta], "batch": [round(x, 4) for x in tb]})
        print(json.dumps(rec), flush=True)
        del coeffs0, coeffs, tools, rng_s, rng_b, pred_s, pred_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

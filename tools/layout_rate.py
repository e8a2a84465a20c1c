"""The layout pipeline's tick (include/heaac_pipeline.h, second half: heaac_layout_pipeline_*): n streams of one
multi-element layout, access units in host memory in, interleaved int16 PCM in host memory out, every tick collected
before the next is submitted.  The units are written the way tests/test_layout_pipeline_gpu.py writes them, for a few
distinct streams that are replicated over the batch (every stream still has its own parser and decoder state); the
pointer arrays of every tick are built once.  Workloads:
  lc_5_1   5.1 AAC-LC (SCE, CPE, CPE, LFE)
  he_5_1   the same layout with explicit SBR per element
  coupled  a program-config HE-AAC layout (SCE, CPE, LFE) with two coupling channel elements whose coupling point is
           drawn per stream and unit -- in the spectrum and AFTER_IMDCT -- and whose gain lists land on either channel
           of the CPE, so that a tick mixes target channels behind SBR
each with the given shares of damaged units (mutated as tests/test_damaged_streams_gpu.py mutates them; the first
tick stays whole: it sets the pipeline's element order).
One JSON line per workload and share: ms per tick (median over the timed ticks, after the warm-up ticks), the stream
count, a SHA-256 over every tick's PCM bytes and status array (warm-up ticks included), and LIB_OVERRIDDEN -- a run
against another library through HEAAC_LIB_PATH says so.
usage: python tools/layout_rate.py [--workloads lc_5_1,he_5_1,coupled] [--damaged 0,0.1] [--streams 1024]
                                   [--distinct 16] [--ticks 16] [--warmup 3] [--threads 0]"""
import argparse, ctypes as C, hashlib, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("ffmpeg-heaac_amd")
import test_layout_gpu as LG
import test_layout_pipeline_gpu as LP
from test_damaged_streams_gpu import _mutate

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", default="lc_5_1,he_5_1,coupled")
ap.add_argument("--damaged", default="0,0.1")
ap.add_argument("--streams", type=int, default=1024)
ap.add_argument("--distinct", type=int, default=16)
ap.add_argument("--ticks", type=int, default=16)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--threads", type=int, default=0)
args = ap.parse_args()
total = args.warmup + args.ticks


def written(workload):
    """(aac configuration, layout, units[tick][distinct stream])"""
    if workload == "coupled":
        _, m4, layout, _, _, unit = LP._coupled_streams(pkg, "he_three_all", 11, args.distinct)
        return m4, layout, [[unit(j) for j in range(args.distinct)] for _ in range(total)]
    rng = np.random.default_rng(sum(map(ord, workload)))
    streams = [LP._stream_units(pkg, rng, workload, total) for _ in range(args.distinct)]
    _, aot, si, cc, he = streams[0]
    r, m4, layout = pkg.asc_layout(LG._asc(aot, si, cc, he=he))
    assert r == 0
    if not he:
        m4.sbr = 0
    return m4, layout, [[streams[j][0][t] for j in range(args.distinct)] for t in range(total)]


def run(workload, share, m4, layout, units):
    n, d = args.streams, args.distinct
    rng = np.random.default_rng(int(share * 1000) + 1)
    pool = [u for tick in units for u in tick]
    ticks = []
    for t in range(total):
        # a damaged unit is one stream's alone: the copies of a distinct stream part ways there
        aus = [units[t][i % d] for i in range(n)]
        for i in range(n if t and share else 0):
            if rng.random() < share:
                aus[i] = _mutate(rng, aus[i], pool)
        keep = {id(a): C.create_string_buffer(a, len(a)) for a in aus}
        ptrs = (C.c_char_p * n)(*[C.cast(keep[id(a)], C.c_char_p) for a in aus])
        sizes = (C.c_int * n)(*[len(a) for a in aus])
        ticks.append((keep, ptrs, sizes))
    pl = pkg.LayoutPipeline(m4, layout, n, threads=args.threads)
    status = np.zeros(n, np.int32)
    sha, ms = hashlib.sha256(), []
    for t in range(total):
        t0 = time.perf_counter()
        pl.submit_raw(ticks[t][1], ticks[t][2], status)
        pcm = pl.collect()
        ms.append((time.perf_counter() - t0) * 1e3)
        sha.update(pcm.tobytes()); sha.update(status.tobytes())
        failed = int((status < 0).sum())
    pl.close()
    timed = ms[args.warmup:]
    print(json.dumps(dict(tool="layout_rate", workload=workload, damaged=share, streams=n, distinct=d, channels=pl.ch,
                          ticks=args.ticks, warmup=args.warmup, ms_per_tick=float(np.median(timed)),
                          ms_min=float(min(timed)), ms_max=float(max(timed)), failed_last_tick=failed,
                          sha256=sha.hexdigest(), LIB_OVERRIDDEN=pkg.LIB_OVERRIDDEN)), flush=True)


for w in args.workloads.split(","):
    what = written(w)
    for share in args.damaged.split(","):
        run(w, float(share), *what)

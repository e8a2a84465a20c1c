"""Bitstream in, int16 PCM out, through host memory: what a caller that does NOT keep its data on the device gets
(PCIe-inclusive -- never the bench's `value`).  n HE-AACv2 streams, one access unit each per tick, through
include/heaac_pipeline.h: host parse (persistent pool) || H2D (pinned) || spectral tools + decode || D2H, consecutive
ticks overlapped.  Prints the stage times of a tick and the end-to-end rate with four ticks in flight, and the
rate when every tick is collected before the next is submitted (no overlap).
frames per tick = T > 1: every tick carries T consecutive access units of each stream (heaac_pipeline_create_streams:
the streams calls on the GPU); 1 is the one-unit tick.  The distinct streams written are 256 / T (at least 16), so that
the units written stay about the same.
--device-parse: the host-parse and the device-parse form (heaac_pipeline_create_ex, HEAAC_PIPELINE_DEVICE_PARSE) of the
same pipeline on the same units, run in turn `--rounds` times (default 3) in this one process; one JSON line per form
with the median rate, every round's rate, the stage times of the median round and parse_counts().  For the device-parse
form the stage named "parse" is submit's host time (pack, the wait for the parse kernel, the host parser's part) and
"h2d" the copy-in stream's (upload, parse kernels, fix-up).
--no-pulses: units without pulse data, which the device parser leaves to the host (the bit writer draws it for about
four units in ten; encoders rarely use it).
usage: python tools/e2e_rate.py [n streams] [ticks] [threads] [frames per tick] [--device-parse] [--rounds R] [--no-pulses]"""
import contextlib, ctypes as C, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("ffmpeg-heaac_amd")
import parse_device_common as PC
import sbr_bitwriter as SW
import test_parse as TP
import test_sbr_parse as TS

argv = list(sys.argv[1:])
both = "--device-parse" in argv
no_pulses = "--no-pulses" in argv
rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 3
if "--rounds" in argv:
    del argv[argv.index("--rounds"):argv.index("--rounds") + 2]
argv = [a for a in argv if not a.startswith("--")]
n = int(argv[0]) if len(argv) > 0 else 32768
ticks = int(argv[1]) if len(argv) > 1 else 12
threads = int(argv[2]) if len(argv) > 2 else 0
T = int(argv[3]) if len(argv) > 3 else 1
rng = np.random.default_rng(5)
cfg = TS._he_cfg(pkg, 1, True)
# 256 distinct streams written once, replicated over the batch (every stream still has its own parser state)
base = 256 if T == 1 else max(16, 256 // T)
writers = [SW.SbrStreamWriter(pkg, 1, ps=True, ps_modes="20") for _ in range(base)]
frames = []
for t in range(ticks):
    aus = []                                  # unit u of writer w at w * T + u
    for w in writers:
        for _ in range(T):
            bits, _ = w.frame(rng)
            with PC.no_pulses() if no_pulses else contextlib.nullcontext():
                aus.append(TP._write_au(rng, 6, 2, False, extras=False, sbr=(bits, False), quiet=True)[0])
    keep = [C.create_string_buffer(a, len(a)) for a in aus]
    ptrs = (C.c_char_p * (n * T))(*[C.cast(keep[(i % base) * T + u], C.c_char_p) for i in range(n) for u in range(T)])
    sizes = (C.c_int * (n * T))(*[len(aus[(i % base) * T + u]) for i in range(n) for u in range(T)])
    frames.append((keep, ptrs, sizes, float(np.mean([len(a) for a in aus]))))


def run(overlap, device_parse=False):
    pl = pkg.Pipeline(cfg, pkg.CFG_HEV2, n, threads=threads, frames_per_tick=T, device_parse=device_parse)
    stage = dict(parse=0.0, h2d=0.0, gpu=0.0, d2h=0.0)
    pl.submit_raw(frames[0][1], frames[0][2]); pl.collect()          # warm-up tick (first-touch, table upload)
    t0 = time.perf_counter()
    if overlap:
        depth, done = 4, 1
        for t in range(1, ticks):
            if t - done >= depth:
                pl.collect(); done += 1
                for k, v in pl.timing().items():
                    stage[k] += v
            pl.submit_raw(frames[t][1], frames[t][2])
        while done < ticks:
            pl.collect(); done += 1
            for k, v in pl.timing().items():
                stage[k] += v
    else:
        for t in range(1, ticks):
            pl.submit_raw(frames[t][1], frames[t][2])
            pl.collect()
            for k, v in pl.timing().items():
                stage[k] += v
    dt = time.perf_counter() - t0
    cnt = ticks - 1
    counts[device_parse] = pl.parse_counts()
    pl.close()
    return (ticks - 1) * n * T / dt, {k: v / cnt for k, v in stage.items()}


counts = {}
if not both:
    rate_seq, st_seq = run(False)
    rate_ovl, st_ovl = run(True)
    out = dict(streams=n, frames_per_tick=T, ticks=ticks, mean_access_unit_bytes=frames[0][3], host_threads=os.cpu_count(),
               stage_ms_per_tick=st_seq, stage_ms_per_tick_overlapped=st_ovl,
               frames_per_s_back_to_back=rate_seq, frames_per_s_overlapped=rate_ovl,
               note="PCIe-inclusive end-to-end rate of a host-buffer caller; not the bench metric")
    print(json.dumps(out))
    sys.exit(0)

# both forms in turn, `rounds` times: host, device, host, device, ...
res = {False: [], True: []}
for _ in range(rounds):
    for dp in (False, True):
        res[dp].append((run(False, dp), run(True, dp)))
for dp in (False, True):
    order = sorted(range(rounds), key=lambda r: res[dp][r][1][0])
    (rate_seq, st_seq), (rate_ovl, st_ovl) = res[dp][order[rounds // 2]]
    out = dict(form="device-parse" if dp else "host-parse", streams=n, frames_per_tick=T, ticks=ticks, pulse_data=not no_pulses,
               mean_access_unit_bytes=frames[0][3], parser_threads=threads, rounds=rounds,
               stage_ms_per_tick=st_seq, stage_ms_per_tick_overlapped=st_ovl,
               frames_per_s_back_to_back=rate_seq, frames_per_s_overlapped=rate_ovl,
               frames_per_s_overlapped_rounds=[r[1][0] for r in res[dp]],
               frames_per_s_back_to_back_rounds=[r[0][0] for r in res[dp]],
               parse_counts=dict(zip(("device", "host"), counts[dp])),
               note="PCIe-inclusive end-to-end rate of a host-buffer caller; not the bench metric; median round of "
                    "both forms run in turn in one process")
    print(json.dumps(out), flush=True)

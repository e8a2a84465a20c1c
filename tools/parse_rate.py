"""Parser throughput.

  python tools/parse_rate.py [n]
      host parser: whole HE-AAC access units (core element + SBR payload with PS) per second through
      heaac_heaac_parse_batch, on 1 thread and on all cores.

  python tools/parse_rate.py --device [--units 32768] [--rounds 12] [--corpus FILE.npz] [--out FILE.jsonl]
      heaac_aac_parse_device against the host parser on the same box, A/B alternating in one process: about 1 024
      distinct in-scope stereo AAC-LC units from the bit writer (FILE.npz is read if it exists, written otherwise),
      tiled to --units.  Timed per round: the device call (device time from events; the H2D of the bytes is timed apart),
      and heaac_aac_parse_batch on 16 threads plus the H2D of its records from pinned memory (host clock around work
      that ends in a synchronise).  One JSON line per form: ms per call over the rounds (median, min, max), bytes over
      the link per unit, and for the device form a nominal store rate: the record sizes (an upper bound of what the kernels write; the
      counter is rocprofv3 --pmc WRITE_SIZE, in a run of its own) over the call time.

  python tools/parse_rate.py --device --he [--units 32768] [--distinct 256] [--rounds 12] [--out FILE.jsonl]
      heaac_heaac_parse_device (the AAC walk and the SBR / PS payload walk, four kernels) against
      heaac_heaac_parse_batch on 16 host threads plus the upload of all its records, the HeaacSbrFrame / HeaacPsFrame
      among them, A/B alternating in one process.  Two corpora from tests/sbr_bitwriter.py, one after the other: stereo
      (coupled and not) and mono + PS HE units, each stream in steady state -- its first header parsed on the host
      ahead of the timing, the timed unit without a header change -- tiled to --units.  Two JSON lines per corpus.

  python tools/parse_rate.py --device [--he] --frames-per-stream T [--units 32768] [--distinct 128] [--rounds 12] [--out FILE.jsonl]
      the streams call (heaac_aac_parse_device_streams, with --he heaac_heaac_parse_device_streams on a mono + PS and a
      stereo corpus) against T chained one-unit calls over the same S = units / T streams, A/B alternating in one
      process, warmed up at the timed shape, the bytes on the device ahead of the timing.  Every stream is in steady
      state and in scope, so both forms take every unit.  The chained form's per-position outputs stay where its calls
      leave them: the re-layout to [S][T] a caller of it still owes is NOT in its time.  Records and final states of
      the two forms are compared byte for byte.  Two JSON lines per corpus: ms per form over the rounds, launches,
      state-row bytes moved by construction, the deferred count, records_equal."""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
pkg = importlib.import_module("ffmpeg-heaac_amd")
import sbr_bitwriter as SW
import test_parse as TP
import test_sbr_parse as TS

def device_mode(argv):
    import argparse, ctypes as C, json
    import torch
    import parse_device_common as PC
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--units", type=int, default=32768)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--corpus", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if a.corpus and os.path.exists(a.corpus):
        z = np.load(a.corpus)
        units = [bytes(z["bytes"][z["off"][i]:z["off"][i + 1]]) for i in range(len(z["off"]) - 1)]
    else:
        units = PC.in_scope_steps(np.random.default_rng(2024), 3, 2, True, a.distinct, 1, adts=0.0, sbr=0.0)[0]
        if a.corpus:
            b, o = pkg.pack_units(units)
            np.savez(a.corpus, bytes=b, off=o)
    n = a.units
    aus = [units[i % len(units)] for i in range(n)]
    mean_size = float(np.mean([len(u) for u in aus]))
    cfg = TP._cfg(pkg, 2, 3, 2)
    assert torch.cuda.is_available(), "parse_rate --device needs a GPU"
    dev = pkg.Device()
    buf, off = pkg.pack_units(aus)
    h_buf = torch.from_numpy(buf).pin_memory()
    h_off = torch.from_numpy(off.astype(np.int32)).pin_memory()
    d_buf = torch.empty_like(h_buf, device="cuda"); d_off = torch.empty_like(h_off, device="cuda")
    d_st = torch.zeros(n * pkg.AAC_STREAM_DT.itemsize, dtype=torch.uint8, device="cuda")
    d_out = dict(coeffs=torch.empty((n, 2, 1024), dtype=torch.float32, device="cuda"),
                 ics=torch.empty(n * 8, dtype=torch.uint8, device="cuda"),
                 tools=torch.empty(n * pkg.TOOLS_FRAME_DT.itemsize, dtype=torch.uint8, device="cuda"),
                 info=torch.empty(n * pkg.AAC_INFO_DT.itemsize, dtype=torch.uint8, device="cuda"),
                 status=torch.empty(n, dtype=torch.int32, device="cuda"))
    # host form: pinned records, the marshalled unit pointers of heaac_aac_parse_batch
    h_out = dict(coeffs=torch.empty((n, 2, 1024), dtype=torch.float32).pin_memory(),
                 ics=torch.empty(n * 8, dtype=torch.uint8).pin_memory(),
                 tools=torch.empty(n * pkg.TOOLS_FRAME_DT.itemsize, dtype=torch.uint8).pin_memory(),
                 info=torch.empty(n * pkg.AAC_INFO_DT.itemsize, dtype=torch.uint8).pin_memory(),
                 status=torch.empty(n, dtype=torch.int32).pin_memory())
    u_out = {k: torch.empty_like(v, device="cuda") for k, v in h_out.items()}
    keep = [C.create_string_buffer(u, len(u)) for u in units]
    ptrs = (C.c_char_p * n)(*[C.cast(keep[i % len(units)], C.c_char_p) for i in range(n)])
    sizes = (C.c_int * n)(*[len(u) for u in aus])
    h_st = np.zeros(n, pkg.AAC_STREAM_DT)
    L = pkg.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())

    def host_round():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        failed = L.heaac_aac_parse_batch(C.byref(cfg), h_st.ctypes.data_as(C.c_void_p), ptrs, sizes, C.c_size_t(n),
                                         vp(h_out["coeffs"]), vp(h_out["ics"]), vp(h_out["tools"]), vp(h_out["info"]),
                                         vp(h_out["status"]), C.c_int(a.threads))
        t1 = time.perf_counter()
        for k in h_out:
            u_out[k].copy_(h_out[k], non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert failed == 0
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def device_round():
        torch.cuda.synchronize()
        ev[0].record()
        d_buf.copy_(h_buf, non_blocking=True); d_off.copy_(h_off, non_blocking=True)
        ev[1].record()
        dev.aac_parse(cfg, d_st, d_buf, d_off, coeff_channels=2, **d_out)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[1].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1])

    for _ in range(3):                                         # warm-up of both forms at the timed shape
        device_round(); host_round()
    assert not d_out["status"].cpu().numpy().any(), "the corpus is in scope: nothing may be deferred"
    same = all(np.array_equal(d_out[k].cpu().numpy().reshape(-1).view(np.uint8), u_out[k].cpu().numpy().reshape(-1).view(np.uint8))
               for k in ("coeffs", "ics", "tools", "info"))
    dev_ms, dev_h2d, host_ms, host_h2d = [], [], [], []
    for _ in range(a.rounds):
        x, y = device_round(); dev_ms.append(x); dev_h2d.append(y)
        x, y = host_round(); host_ms.append(x); host_h2d.append(y)
    rec = 2 * 4096 + 8 + pkg.TOOLS_FRAME_DT.itemsize + pkg.AAC_INFO_DT.itemsize + 4
    # an upper bound from the record sizes, not a counter: the zero fill, then every record as if the walk wrote all of it
    # (it writes the coefficient rows whole, of the tools record only the fields the unit uses)
    stored = rec + pkg.TOOLS_FRAME_DT.itemsize + pkg.AAC_STREAM_DT.itemsize
    sp = lambda v: dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))
    lines = [
        dict(form="heaac_aac_parse_device", units=n, distinct=len(units), mean_unit_bytes=round(mean_size, 1), rounds=a.rounds,
             call_ms=sp(dev_ms), h2d_bytes_ms=sp(dev_h2d), link_bytes_per_unit=round(mean_size + 4, 1),
             nominal_stored_bytes_per_unit=stored, nominal_store_GBps=round(stored * n / (np.median(dev_ms) * 1e-3) / 1e9, 1),
             units_per_s=round(n / (np.median(dev_ms) * 1e-3)), records_equal_host=bool(same)),
        dict(form="heaac_aac_parse_batch + H2D", units=n, threads=a.threads, rounds=a.rounds,
             parse_ms=sp(host_ms), h2d_records_ms=sp(host_h2d), total_ms=sp([x + y for x, y in zip(host_ms, host_h2d)]),
             link_bytes_per_unit=rec, units_per_s=round(n / ((np.median(host_ms) + np.median(host_h2d)) * 1e-3))),
    ]
    for l in lines:
        print(json.dumps(l))
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


def he_mode(argv):
    import argparse, ctypes as C, json
    import torch
    import sbr_device_common as SD
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--he", action="store_true")
    ap.add_argument("--units", type=int, default=32768)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "parse_rate --device needs a GPU"
    dev = pkg.Device()
    L = pkg.lib()
    n = a.units
    vp = lambda t: C.c_void_p(t.data_ptr())
    sp = lambda v: dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))
    lines = []
    for cpe in (True, False):
        rng = np.random.default_rng(2025 + cpe)
        cfg = SD.he_cfg(pkg, cpe)
        with_ps = not cpe
        d = a.distinct
        writers = SD.make_writers(pkg, d, cpe)
        tab = pkg.SbrHeaderTable(256)
        st0, sst0 = np.zeros(d, pkg.AAC_STREAM_DT), pkg.sbr_streams(d)
        first = pkg.heaac_parse_batch(cfg, st0, sst0, tab, SD.he_units(rng, writers, cpe), with_ps=with_ps)
        assert first["failed"] == 0
        units = SD.he_units(rng, writers, cpe)                 # the timed units: no header, from the states st0 / sst0
        tile = np.arange(n) % d
        aus = [units[i] for i in tile]
        mean_size = float(np.mean([len(u) for u in aus]))
        hdr = tab.headers()
        d_hdr = pkg.to_device(hdr)
        buf, off = pkg.pack_units(aus)
        h_buf = torch.from_numpy(buf).pin_memory()
        h_off = torch.from_numpy(off.astype(np.int32)).pin_memory()
        d_buf = torch.empty_like(h_buf, device="cuda"); d_off = torch.empty_like(h_off, device="cuda")
        d_st0 = pkg.to_device(st0[tile]); d_st = torch.empty_like(d_st0)
        d_sst_in = pkg.to_device(sst0[tile]); d_sst_out = torch.empty_like(d_sst_in)
        sizes_of = dict(coeffs=(n, 2, 1024), ics=n * 8, tools=n * pkg.TOOLS_FRAME_DT.itemsize, info=n * pkg.AAC_INFO_DT.itemsize,
                        status=n, sbr=n * pkg.SBR_FRAME_DT.itemsize, ps=n * pkg.PS_FRAME_DT.itemsize)
        dt_of = dict(coeffs=torch.float32, status=torch.int32)
        names = [k for k in sizes_of if with_ps or k != "ps"]
        d_out = {k: torch.empty(sizes_of[k], dtype=dt_of.get(k, torch.uint8), device="cuda") for k in names}
        h_out = {k: torch.empty(sizes_of[k], dtype=dt_of.get(k, torch.uint8)).pin_memory() for k in names}
        u_out = {k: torch.empty_like(v, device="cuda") for k, v in h_out.items()}
        for t in list(d_out.values()) + list(h_out.values()):  # one fill on both sides: a byte neither form writes compares equal
            t.view(-1).view(torch.uint8).fill_(0xA5)
        keep = [C.create_string_buffer(u, len(u)) for u in units]
        ptrs = (C.c_char_p * n)(*[C.cast(keep[i], C.c_char_p) for i in tile])
        sizes = (C.c_int * n)(*[len(u) for u in aus])
        h_st0, h_sst0 = st0[tile].copy(), sst0[tile].copy()
        h_st, h_sst = h_st0.copy(), h_sst0.copy()

        def host_round():
            h_st[...] = h_st0; h_sst[...] = h_sst0            # the same units from the same states every round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            failed = L.heaac_heaac_parse_batch(C.byref(cfg), h_st.ctypes.data_as(C.c_void_p), h_sst.ctypes.data_as(C.c_void_p),
                                               C.c_void_p(tab._h), ptrs, sizes, C.c_size_t(n), vp(h_out["coeffs"]), vp(h_out["ics"]),
                                               vp(h_out["tools"]), vp(h_out["sbr"]), vp(h_out["ps"]) if with_ps else None,
                                               vp(h_out["info"]), vp(h_out["status"]), C.c_int(a.threads))
            t1 = time.perf_counter()
            for k in h_out:
                u_out[k].copy_(h_out[k], non_blocking=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert failed == 0
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3

        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

        def device_round():
            d_st.copy_(d_st0)
            torch.cuda.synchronize()
            ev[0].record()
            d_buf.copy_(h_buf, non_blocking=True); d_off.copy_(h_off, non_blocking=True)
            ev[1].record()
            dev.heaac_parse_device(cfg, d_st, d_sst_in, d_buf, d_off, d_hdr, coeff_channels=2, sst_out=d_sst_out,
                                   **{k: d_out[k] for k in names})
            ev[2].record()
            torch.cuda.synchronize()
            return ev[1].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1])

        for _ in range(3):
            device_round(); host_round()
        deferred = int(d_out["status"].cpu().numpy().astype(bool).sum())
        differ = [k for k in names if not np.array_equal(d_out[k].cpu().numpy().reshape(-1).view(np.uint8),
                                                         u_out[k].cpu().numpy().reshape(-1).view(np.uint8))]
        if not np.array_equal(d_sst_out.cpu().numpy().reshape(-1), h_sst.reshape(-1)):     # (the two arrays differ in shape)
            differ.append("sst")
        same = deferred == 0 and not differ
        dev_ms, dev_h2d, host_ms, host_h2d = [], [], [], []
        for _ in range(a.rounds):
            x, y = device_round(); dev_ms.append(x); dev_h2d.append(y)
            x, y = host_round(); host_ms.append(x); host_h2d.append(y)
        rec = sum(int(np.prod(sizes_of[k])) * (4 if k in dt_of else 1) for k in names) // n
        corpus = "stereo" if cpe else "mono_ps"
        lines += [
            dict(form="heaac_heaac_parse_device", corpus=corpus, units=n, distinct=d, mean_unit_bytes=round(mean_size, 1),
                 rounds=a.rounds, call_ms=sp(dev_ms), h2d_bytes_ms=sp(dev_h2d), link_bytes_per_unit=round(mean_size + 4, 1),
                 units_per_s=round(n / (np.median(dev_ms) * 1e-3)), deferred=deferred, records_equal_host=bool(same), records_that_differ=differ),
            dict(form="heaac_heaac_parse_batch + H2D", corpus=corpus, units=n, threads=a.threads, rounds=a.rounds,
                 parse_ms=sp(host_ms), h2d_records_ms=sp(host_h2d), total_ms=sp([x + y for x, y in zip(host_ms, host_h2d)]),
                 link_bytes_per_unit=rec, units_per_s=round(n / ((np.median(host_ms) + np.median(host_h2d)) * 1e-3))),
        ]
    for l in lines:
        print(json.dumps(l))
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


def streams_mode(argv):
    import argparse, json
    import torch
    import parse_device_common as PC
    import sbr_device_common as SD
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--he", action="store_true")
    ap.add_argument("--frames-per-stream", type=int, required=True)
    ap.add_argument("--units", type=int, default=32768)
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "parse_rate --device needs a GPU"
    dev = pkg.Device()
    T = a.frames_per_stream
    S = a.units // T
    n = S * T
    d = min(a.distinct, S)
    sp = lambda v: dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))
    row = int(pkg.sbr_streams(1).shape[1])
    lines = []
    for corpus in (("mono_ps", "stereo") if a.he else ("aac_lc_stereo",)):
        cpe = corpus != "mono_ps"
        rng = np.random.default_rng(2026 + cpe + 10 * T)
        if a.he:
            cfg, cc, with_ps = SD.he_cfg(pkg, cpe), 2 if cpe else 1, not cpe
            writers = SD.make_writers(pkg, d, cpe)
            tab = pkg.SbrHeaderTable(256)
            st0, sst0 = np.zeros(d, pkg.AAC_STREAM_DT), pkg.sbr_streams(d)
            for _ in range(2):                                 # the first headers: the host's
                first = pkg.heaac_parse_batch(cfg, st0, sst0, tab, SD.he_units(rng, writers, cpe), with_ps=with_ps)
                assert first["failed"] == 0
            rows = [SD.he_units(rng, writers, cpe) for _ in range(T)]
            d_hdr = pkg.to_device(tab.headers())
        else:
            cfg, cc, with_ps = TP._cfg(pkg, 2, 3, 2), 2, False
            rows = PC.in_scope_steps(rng, 3, 2, True, d, T, adts=0.0, sbr=0.0)
            st0, sst0 = np.zeros(d, pkg.AAC_STREAM_DT), None
        tile = np.arange(S) % d
        mean_size = float(np.mean([len(u) for r in rows for u in r]))
        # the bytes of both layouts on the device ahead of the timing: [S][T] for the streams call, [S] per position
        def up(aus):
            b, o = pkg.pack_units(aus)
            return torch.from_numpy(np.concatenate([b, np.zeros(4, np.uint8)])).cuda(), torch.from_numpy(o.astype(np.int32)).cuda()
        d_buf, d_off = up([rows[t][i] for i in tile for t in range(T)])
        pos = [up([rows[t][i] for i in tile]) for t in range(T)]
        d_st0 = pkg.to_device(st0[tile])
        d_st = [torch.empty_like(d_st0) for _ in range(2)]
        sizes_of = dict(coeffs=cc * 1024, ics=cc * pkg.ICS_DT.itemsize, tools=pkg.TOOLS_FRAME_DT.itemsize, info=pkg.AAC_INFO_DT.itemsize, status=1)
        if a.he:
            sizes_of.update(sbr=pkg.SBR_FRAME_DT.itemsize)
            if with_ps:
                sizes_of.update(ps=pkg.PS_FRAME_DT.itemsize)
            d_sst0 = pkg.to_device(sst0[tile])
            d_sst = [torch.empty_like(d_sst0) for _ in range(3)]       # streams out; the chained form's ping and pong
        dt_of = dict(coeffs=torch.float32, status=torch.int32)
        mk = lambda units: {k: torch.empty(units * v, dtype=dt_of.get(k, torch.uint8), device="cuda") for k, v in sizes_of.items()}
        s_out = mk(n)
        s_out.update(taken=torch.empty(S, dtype=torch.int32, device="cuda"), hold=torch.empty(n, dtype=torch.uint8, device="cuda"))
        c_out = [mk(S) for _ in range(T)]
        for t in list(s_out.values()) + [v for o in c_out for v in o.values()]:       # one fill on both sides
            t.view(torch.uint8).fill_(0xA5)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def streams_round():
            d_st[0].copy_(d_st0)
            torch.cuda.synchronize()
            ev[0].record()
            if a.he:
                dev.heaac_parse_device_streams(cfg, d_st[0], d_sst0, d_buf, d_off, d_hdr, T, coeff_channels=cc, sst_out=d_sst[0], **s_out)
            else:
                dev.aac_parse_streams(cfg, d_st[0], d_buf, d_off, T, coeff_channels=cc, **s_out)
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        def chained_round():
            d_st[1].copy_(d_st0)
            torch.cuda.synchronize()
            ev[0].record()
            for t in range(T):
                if a.he:
                    dev.heaac_parse_device(cfg, d_st[1], d_sst0 if t == 0 else d_sst[1 + (t - 1) % 2], pos[t][0], pos[t][1], d_hdr,
                                           coeff_channels=cc, sst_out=d_sst[1 + t % 2], **c_out[t])
                else:
                    dev.aac_parse(cfg, d_st[1], pos[t][0], pos[t][1], coeff_channels=cc, **c_out[t])
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        for _ in range(3):                                     # warm-up of both forms at the timed shape
            streams_round(); chained_round()
        deferred_s = int((T - s_out["taken"].cpu().numpy().astype(np.int64)).sum())
        deferred_c = int(sum(o["status"].cpu().numpy().astype(bool).sum() for o in c_out))
        differ = []
        for k, size in sizes_of.items():
            x = s_out[k].view(S, T, size)
            if any(not torch.equal(x[:, t], c_out[t][k].view(S, size)) for t in range(T)):
                differ.append(k)
        if not torch.equal(d_st[0], d_st[1]):
            differ.append("st")
        if a.he and not torch.equal(d_sst[0], d_sst[1 + (T - 1) % 2]):
            differ.append("sst")
        if s_out["hold"].any():
            differ.append("hold")
        same = deferred_s == 0 and deferred_c == 0 and not differ
        s_ms, c_ms = [], []
        for _ in range(a.rounds):
            s_ms.append(streams_round()); c_ms.append(chained_round())
        common = dict(corpus=corpus, streams=S, frames_per_stream=T, units=n, distinct_streams=d, mean_unit_bytes=round(mean_size, 1),
                      rounds=a.rounds)
        name = "heaac_heaac_parse_device" if a.he else "heaac_aac_parse_device"
        lines += [
            dict(form=name + "_streams", **common, call_ms=sp(s_ms), units_per_s=round(n / (np.median(s_ms) * 1e-3)),
                 launches=2, state_row_bytes_moved=4 * row * S if a.he else 0, deferred=deferred_s, records_equal=bool(same),
                 records_that_differ=differ),
            dict(form="%d x %s" % (T, name), **common, call_ms=sp(c_ms), units_per_s=round(n / (np.median(c_ms) * 1e-3)),
                 launches=(4 if a.he else 2) * T, state_row_bytes_moved=4 * row * n if a.he else 0, deferred=deferred_c,
                 relayout_to_S_T_in_time=False),
        ]
    for l in lines:
        print(json.dumps(l))
    if a.out:
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if "--device" in sys.argv:
    (streams_mode if "--frames-per-stream" in sys.argv else he_mode if "--he" in sys.argv else device_mode)(sys.argv[1:])
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
rng = np.random.default_rng(1)
cfg = TS._he_cfg(pkg, 1, True)
writers = [SW.SbrStreamWriter(pkg, 1, ps=True, ps_modes="20") for _ in range(n)]
frames = []
for step in range(3):
    aus = []
    for w in writers:
        bits, _ = w.frame(rng)
        aus.append(TP._write_au(rng, 6, 2, False, extras=False, sbr=(bits, False), quiet=True)[0])
    frames.append(aus)
print("mean access unit: %.0f bytes" % np.mean([len(a) for f in frames for a in f]))
import ctypes as C
L = pkg.lib()
marsh = []
for aus in frames:
    keep = [C.create_string_buffer(bytes(a), len(a)) for a in aus]
    marsh.append((keep, (C.c_char_p * n)(*[C.cast(k, C.c_char_p) for k in keep]), (C.c_int * n)(*[len(a) for a in aus])))
coeffs = np.zeros((n, 2, 1024), np.float32); ics = np.zeros((n, 2), pkg.ICS_DT); tools = np.zeros(n, pkg.TOOLS_FRAME_DT)
sbr = np.zeros(n, pkg.SBR_FRAME_DT); ps = np.zeros(n, pkg.PS_FRAME_DT); status = np.zeros(n, np.int32)
p_ = lambda a: a.ctypes.data_as(C.c_void_p)
for threads in (1, 2, 4, os.cpu_count()):
    best = 0.0
    for rep in range(5):
        tab = pkg.SbrHeaderTable(4096)
        st = np.zeros(n, pkg.AAC_STREAM_DT); sst = pkg.sbr_streams(n)
        t0 = time.perf_counter()
        for keep, ptrs, sizes in marsh:
            failed = L.heaac_heaac_parse_batch(C.byref(cfg), p_(st), p_(sst), C.c_void_p(tab._h), ptrs, sizes, C.c_size_t(n),
                                               p_(coeffs), p_(ics), p_(tools), p_(sbr), p_(ps), None, p_(status), C.c_int(threads))
            assert failed == 0
        dt = time.perf_counter() - t0
        best = max(best, len(marsh) * n / dt)
    print("threads %2d: %.0f access units/s" % (threads, best))

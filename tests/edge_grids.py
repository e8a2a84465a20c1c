"""Structural profiles for the parity campaign (tests/test_grid_reach.py, tests/test_grids_gpu.py).

Host logic only (numpy).  tests/edge_signals.py rewrites values and leaves the structure alone; this module is its
counterpart: it takes the frames of synth.he_stream / lc_stream as they are and rewrites only STRUCTURE -- the SBR time
grid with its noise border and transient pointers, the PS envelope borders, the window sequences -- over the whole
space csrc/validate.h accepts, not only the part of it the synth's chains (or a carry-consistent encoder) produce.
The synth generators and their RNG draws are not touched (bench.py and the golden hashes draw from them); what this
module draws comes from generators of its own.

Every field a parser carries from frame to frame is derived per stream the way csrc/sbr_core.h sc_grid / sc_copy_grid
derive it (class _Carry): bs_freq_res[0], t_env_num_env_old, e_a[0] = -(e_a[1]_prev != L_prev), the stale t_env[] and
bs_freq_res[] entries behind the last border, bs_invf_mode[1]; for PS num_env_old and is34bands_old.  sc_grid reads
the leading border without looking at the previous frame, so a frame that starts later than the last one ended (a gap)
or earlier (an overlap) is an ordinary parsed record.  The `free` profiles draw those carries as well: any record the
validator accepts may reach the kernels through the C ABI.

Scalefactors are redrawn for the new envelope count in the synth's ranges, so the output stays finite
(tests/test_grid_reach.py asserts it).
"""
import numpy as np

from edge_signals import HE_CFGS, SEED                               # noqa: F401  (the campaign's configurations)

SBR_PROFILES = ("five_env", "narrow", "seams", "free")
PS_PROFILES = ("aligned_uneven", "ps_narrow", "ps_free")
PROFILES = SBR_PROFILES + PS_PROFILES
DS_PROFILES = ("five_env", "seams")                                  # these also run on the downsampled bank

STREAMS = 24
STEPS = 8
SEAM_P_SWITCH = 0.25                                                 # seams: resets on some of the frames

# the header with m = 48 and the widest limiter table (n_lim = 10) of the whole header space;
# tests/test_grid_reach.py searches the space and asserts both
WIDEST_LIMITER = dict(sample_rate=24000, start_freq=1, stop_freq=12, xover=0, freq_scale=0, alter_scale=0,
                      noise_bands=2, limiter_bands=3)
WIDEST_N_LIM = 10

# narrow: one-slot envelopes at either end and in a row, the longest and the shortest frame.  Validator space, not
# syntax space: [3, 4, 5, 6, 7, 19] has no sbr_grid() spelling (relative borders step by 2 at least), the C ABI takes it
NARROW_GRIDS = ([0, 1, 9, 17], [2, 10, 18, 19], [3, 4, 5, 6, 7, 19], [0, 19], [3, 16], [0, 1, 2, 3, 4, 16],
                [2, 14, 15, 16, 17, 18], [0, 1, 18, 19])

# aligned_uneven: every border at 8k - 1, and not what frame class 0 gives ([-1, 31], [-1, 15, 31],
# [-1, 7, 15, 23, 31]): the other five subsets of {7, 15, 23}
ALIGNED_UNEVEN = ([-1, 7, 31], [-1, 23, 31], [-1, 7, 15, 31], [-1, 7, 23, 31], [-1, 15, 23, 31])
PS_NARROW = ([-1, 0, 31], [-1, 30, 31], [-1, 0, 1, 2, 3, 31], [-1, 27, 28, 29, 30, 31], [-1, 0, 30, 31],
             [-1, 0, 1, 31], [-1, 29, 30, 31], [-1, 0, 1, 29, 30, 31])


def headers(pkg, synth, profile):
    """the campaign's header table; five_env adds the widest-limiter header as the last entry"""
    hdr = synth.default_headers(pkg, extra=True)
    if profile == "five_env":
        hdr = np.concatenate([hdr, pkg.sbr_make_header(**WIDEST_LIMITER)])
    return hdr


# ---------------------------------------------------------------------------
# SBR grids
# ---------------------------------------------------------------------------
class _Carry:
    """what sc_grid / sc_copy_grid read of the previous frame of one channel (a new stream: zeros, e_a[1] = -1)"""

    def __init__(self):
        self.L = 0
        self.t_env = np.zeros(8, np.uint8)
        self.freq_res = np.zeros(8, np.uint8)
        self.e_a1 = -1
        self.invf0 = np.zeros(5, np.uint8)

    def t_old(self):
        return int(self.t_env[self.L])

    def move(self, ch):
        """the previous frame's values move first (sbr_core.h:180-183, 241)"""
        ch["bs_freq_res"][0] = self.freq_res[self.L]
        ch["t_env_num_env_old"] = self.t_env[self.L]
        ch["e_a"][0] = -int(self.e_a1 != self.L)
        ch["bs_invf_mode"][1] = self.invf0

    def keep(self, ch):
        self.L = int(ch["bs_num_env"])
        self.t_env[:] = ch["t_env"]
        self.freq_res[:] = ch["bs_freq_res"]
        self.e_a1 = int(ch["e_a"][1])
        self.invf0 = ch["bs_invf_mode"][0].copy()


def max_pointer(L):
    """bs_pointer has ceil(log2(L + 1)) bits and is refused above L + 1"""
    nbits = 0
    while (1 << nbits) < L + 1:
        nbits += 1
    return min(L + 1, (1 << nbits) - 1)


def noise_border_and_transient(t_env, L, rule, pointer):
    """(t_q[1], e_a[1]) as sc_grid derives them (sbr_core.h:228-245) for a grid whose trailing end is variable
    (rule "trail": FIXVAR, VARVAR) or whose leading end alone is (rule "lead": VARFIX).  t_env: the channel's eight
    entries with this frame's borders written: pointer 0 of "trail" takes the stale entry behind the last border."""
    if rule == "trail":
        idx = L + 1 if pointer == 0 else L - max(pointer - 1, 1)
        l_a = L + 1 - pointer if pointer else -1
    else:
        idx = 1 if pointer == 0 else L - 1 if pointer == 1 else pointer - 1
        l_a = pointer - 1 if pointer > 1 else -1
    return int(t_env[idx]), l_a


def _five_env_borders(rng, lead, trail):
    """VARVAR with five envelopes: lead + n_lead relative borders walking up, trail - n_trail walking down,
    n_lead + n_trail = 4, steps from {2, 4, 6, 8}, the two walks not meeting"""
    while True:
        n_lead = int(rng.integers(1, 4))
        up = lead + np.cumsum(rng.choice([2, 4, 6, 8], n_lead))
        down = trail - np.cumsum(rng.choice([2, 4, 6, 8], 4 - n_lead))
        if up[-1] < down[-1]:
            return [lead] + [int(x) for x in up] + [int(x) for x in down[::-1]] + [trail]


def _inner(rng, lead, trail, L):
    cuts = sorted(rng.choice(np.arange(lead + 1, trail), size=L - 1, replace=False).tolist())
    return [lead] + [int(x) for x in cuts] + [trail]


def _seam_lead(carry, want):
    """a leading border `want` slots off the carry if 0..3 has room for it, else the nearest seam on the other side"""
    for g in (want, -want, 1 if want < 0 else -1):
        if 0 <= carry + g <= 3:
            return carry + g
    raise AssertionError((carry, want))


def _sbr_grid(profile, rng, s, t, carry):
    """the grid of stream s, frame t: dict(t, rule, pointer) or, for `free`, dict(t, free=True)"""
    if profile == "five_env":
        g = dict(t=_five_env_borders(rng, (s + 3 * t) % 4, 16 + (s // 4 + t) % 4), rule="trail", pointer=(s + t) % 7)
    elif profile == "narrow":
        tt = list(NARROW_GRIDS[(s + t) % len(NARROW_GRIDS)])
        L = len(tt) - 1
        g = dict(t=tt, rule="lead" if tt[-1] == 16 and (s + t) % 3 == 0 else "trail",
                 pointer=(s // 2 + t) % (max_pointer(L) + 1))
    elif profile == "seams":
        # gaps of 1, 2, 3 and overlaps of 1, 2, 3 slots in turn; the trailing border is drawn so that the NEXT
        # frame's seam has room (a gap of g needs a carry of at most 3 - g, an overlap of g one of at least g)
        seam = (1, -1, 2, -2, 3, -3)
        lead = _seam_lead(max(carry.t_old() - 16, 0), seam[(s + t) % 6])
        nxt = seam[(s + t + 1) % 6]
        trail = 16 + int(rng.integers(0, 4 - nxt) if nxt > 0 else rng.integers(-nxt, 4))
        L = 1 + (s // 6 + t) % 4
        g = dict(t=_inner(rng, lead, trail, L), rule="trail", pointer=int(rng.integers(0, max_pointer(L) + 1)))
    elif profile == "free":
        L = 1 + (s + t) % 5
        g = dict(t=_inner(rng, int(rng.integers(0, 4)), 16 + int(rng.integers(0, 4)), L), free=True)
    else:
        raise KeyError(profile)
    return g


def _write_grid(ch, carry, g, rng, amp_header):
    """one channel's record from the grid g, through the carry"""
    tt = g["t"]
    L = len(tt) - 1
    carry.move(ch)
    ch["bs_num_env"] = L
    ch["bs_num_noise"] = 2 if L > 1 else 1
    ch["t_env"][:] = carry.t_env                                   # entries behind the last border persist
    ch["t_env"][: L + 1] = tt
    ch["bs_freq_res"][1:] = carry.freq_res[1:]
    ch["bs_freq_res"][1: L + 1] = rng.integers(0, 2, L)
    ch["t_q"][:] = 0
    ch["t_q"][0], ch["t_q"][int(ch["bs_num_noise"])] = tt[0], tt[L]
    if g.get("free"):
        # uniform over heaac_check_sbr_channel: the carries and the pointer-derived fields are free as well
        ch["bs_amp_res"] = int(rng.integers(0, 2))
        ch["bs_freq_res"][:] = rng.integers(0, 2, 8)
        ch["t_env"][L + 1:] = rng.integers(0, 20, 7 - L)
        ch["t_env_num_env_old"] = int(rng.integers(0, 20))
        ch["e_a"][:] = [-int(rng.integers(0, 2)), int(rng.integers(-1, L + 1))]
        if L > 1:
            ch["t_q"][1] = int(rng.integers(0, 20))
    else:
        ch["bs_amp_res"] = amp_header                              # no FIXFIX single envelope among these grids
        tq1, l_a = noise_border_and_transient(ch["t_env"], L, g["rule"], g["pointer"])
        if L > 1:
            ch["t_q"][1] = tq1
        ch["e_a"][1] = l_a


def _write_facs(ch, rng, balance):
    """scalefactors for the new envelope count, in synth._SbrChain's ranges (he_stream's for a balance channel)"""
    L, nq, amp = int(ch["bs_num_env"]), int(ch["bs_num_noise"]), int(ch["bs_amp_res"])
    ch["env_facs_q"][:] = 0
    ch["noise_facs_q"][:] = 0
    if balance:
        ch["env_facs_q"][:L] = rng.integers(0, 25 if amp else 49, (L, 48))
        ch["noise_facs_q"][:nq] = rng.integers(0, 25, (nq, 5))
    else:
        ch["env_facs_q"][:L] = rng.integers(8 if amp else 16, 24 if amp else 47, (L, 48))
        ch["noise_facs_q"][:nq] = rng.integers(4, 12, (nq, 5))


def rewrite_sbr(profile, frames, hdr, ncore, rng):
    """Rewrite the SBR grids of a run in place: frames = the list he_stream yields, one chain per stream."""
    n = frames[0]["sbr"].shape[0]
    carries = [[_Carry() for _ in range(ncore)] for _ in range(n)]
    for t, step in enumerate(frames):
        step["pointer"] = np.full((n, ncore), -1)                  # bs_pointer of each grid drawn (for the counters)
        for s in range(n):
            fr = step["sbr"][s]
            if not fr["start"]:
                # nothing is parsed: the carries stay, the record shows the border the state rows belong to
                for c in range(ncore):
                    fr["ch"][c]["t_env_num_env_old"] = carries[s][c].t_old()
                continue
            amp = int(hdr[int(fr["hdr"])]["bs_amp_res_header"])
            coupled = bool(fr["bs_coupling"])
            g = None
            for c in range(ncore):
                ch, carry = fr["ch"][c], carries[s][c]
                if c and coupled:
                    # sc_copy_grid: its own carries, then every transmitted grid field of the partner
                    c0 = fr["ch"][0]
                    carry.move(ch)
                    for f in ("bs_num_env", "bs_num_noise", "bs_amp_res", "t_env", "t_q"):
                        ch[f] = c0[f]
                    ch["bs_freq_res"][1:] = c0["bs_freq_res"][1:]
                    ch["e_a"][1] = c0["e_a"][1]
                    ch["bs_invf_mode"][0] = c0["bs_invf_mode"][0]
                    if g.get("free"):
                        ch["t_env_num_env_old"] = int(rng.integers(0, 20))
                        ch["e_a"][0] = -int(rng.integers(0, 2))
                        ch["bs_freq_res"][0] = int(rng.integers(0, 2))
                else:
                    g = _sbr_grid(profile, rng, s, t, carry)
                    _write_grid(ch, carry, g, rng, amp)
                    step["pointer"][s, c] = g.get("pointer", -1)
                _write_facs(ch, rng, balance=bool(c and coupled))
                carry.keep(ch)


# ---------------------------------------------------------------------------
# PS grids
# ---------------------------------------------------------------------------
def _ps_borders(profile, rng, s, t):
    if profile == "aligned_uneven":
        return list(ALIGNED_UNEVEN[(s + t) % len(ALIGNED_UNEVEN)])
    if profile == "ps_narrow":
        return list(PS_NARROW[(s + t) % len(PS_NARROW)])
    if profile == "ps_free":
        E = 1 + (s + t) % 5
        return [-1] + sorted(rng.choice(np.arange(0, 31), size=E - 1, replace=False).tolist()) + [31]
    raise KeyError(profile)


def rewrite_ps(profile, frames, rng, ps_mode):
    """Rewrite the PS envelope grids of a run in place; parameters are redrawn for the new envelope count in
    synth._PsChain's ranges.  num_env_old / is34bands_old follow the stream (sc_ps), in ps_free they are free."""
    n = frames[0]["ps"].shape[0]
    num_env = [0] * n
    is34 = [0] * n
    for t, step in enumerate(frames):
        for s in range(n):
            p = step["ps"][s]
            if not p["start"]:
                continue
            b = _ps_borders(profile, rng, s, t)
            E = len(b) - 1
            p["num_env"] = E
            p["border_position"][:] = 0
            p["border_position"][: E + 1] = b
            p["num_env_old"], p["is34bands_old"] = num_env[s], is34[s]
            if profile == "ps_free":
                p["num_env_old"] = int(rng.integers(0, 6))
                p["is34bands_old"] = int(rng.integers(0, 2))
                if ps_mode != "20":                                # (the "20" runs keep IPD / OPD off)
                    p["enable_ipdopd"] = int(rng.integers(0, 2))
            ni, nc, npd = int(p["nr_iid_par"]), int(p["nr_icc_par"]), int(p["nr_ipdopd_par"])
            lim = 15 if p["iid_quant"] else 7
            for f in ("iid_par", "icc_par", "ipd_par", "opd_par"):
                p[f][:] = 0
            p["iid_par"][:E, :ni] = rng.integers(-lim, lim + 1, (E, ni))
            p["icc_par"][:E, :nc] = rng.integers(0, 8, (E, nc))
            if p["enable_ipdopd"]:
                p["ipd_par"][:E, :npd] = rng.integers(0, 8, (E, npd))
                p["opd_par"][:E, :npd] = rng.integers(0, 8, (E, npd))
            num_env[s], is34[s] = E, int(p["is34bands"])


def he_frames(pkg, synth, cfg, profile, n, steps, seed, hdr, ps_mode="20"):
    """synth.he_stream frames (every header of `hdr` in turn, half the HE-AACv1 pairs coupled; seams: header switches
    with their resets) with the structure of `profile`: a list of {coeffs, ics, sbr, ps} per step."""
    rng = np.random.default_rng(seed)
    events = dict(p_switch=SEAM_P_SWITCH) if profile == "seams" else None
    frames = list(synth.he_stream(rng, cfg, n, steps, hdr, ps_mode=ps_mode, hdr_choice=np.arange(n) % len(hdr),
                                  coupling=0.5 if cfg == pkg.CFG_HEV1 else 0.0, events=events))
    own = np.random.default_rng([seed, PROFILES.index(profile)])
    if profile in SBR_PROFILES:
        rewrite_sbr(profile, frames, hdr, 2 if cfg == pkg.CFG_HEV1 else 1, own)
    else:
        assert cfg == pkg.CFG_HEV2, "PS profiles need the PS configuration"
        rewrite_ps(profile, frames, own, ps_mode)
    return frames


def cases():
    """(profile, cfg name, PS mode, downsampled) of the campaign: the SBR profiles in every configuration, the PS
    profiles in the two that run PS; the downsampled bank for DS_PROFILES"""
    out = []
    for profile in PROFILES:
        for cfgname, ps_mode in HE_CFGS:
            if profile in PS_PROFILES and cfgname != "CFG_HEV2":
                continue
            for ds in (False, True) if profile in DS_PROFILES else (False,):
                out.append((profile, cfgname, ps_mode, ds))
    return out


# ---------------------------------------------------------------------------
# window sequences
# ---------------------------------------------------------------------------
WIN_STREAMS = 8
WIN_STEPS = 8


def _de_bruijn_pairs(k):
    """a cyclic sequence over 0..k-1 of length k * k in which every ordered pair (a, b) is adjacent exactly once"""
    a = [0] * (2 * k)
    seq = []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def window_ics(pkg, n, steps, channel):
    """ics [steps][n] of one channel: frame t of stream s goes from state q[s * steps + t] to q[s * steps + t + 1]
    of a cyclic sequence of (window_sequence, window shape) states that has every ordered pair once: with
    n * steps = 64 the run visits all 16 (ws, ws_prev) x 4 (kb, kb_prev) combinations, each stream a true chain (the
    `previous` fields of frame t are frame t - 1's).  Channels walk the cycle from different places."""
    assert n * steps == 64
    q = _de_bruijn_pairs(8)
    assert len(q) == 64 and len({(q[i], q[(i + 1) % 64]) for i in range(64)}) == 64
    out = np.zeros((steps, n), pkg.ICS_DT)
    for s in range(n):
        for t in range(steps):
            i = s * steps + t + 19 * channel
            prev, cur = q[i % 64], q[(i + 1) % 64]
            out[t, s]["window_sequence"] = [cur >> 1, prev >> 1]
            out[t, s]["use_kb_window"] = [cur & 1, prev & 1]
    return out


def _window_coeffs(synth, rng, ics, bins):
    """synth._coeffs per channel: the band limit follows the NEW window sequence"""
    return np.ascontiguousarray(np.stack([synth._coeffs(rng, ics[:, c], bins) for c in range(ics.shape[1])], axis=1))


def lc_window_frames(pkg, synth, channels, seed):
    """[(coeffs, ics)] per step for lc_decode"""
    rng = np.random.default_rng([seed, 100])
    per_ch = [window_ics(pkg, WIN_STREAMS, WIN_STEPS, c) for c in range(channels)]
    out = []
    for t in range(WIN_STEPS):
        ics = np.ascontiguousarray(np.stack([p[t] for p in per_ch], axis=1))
        out.append((_window_coeffs(synth, rng, ics, 1024), ics))
    return out


def he_window_frames(pkg, synth, cfg, seed, hdr, ps_mode="20"):
    """he_stream frames whose CORE walks the window chains (SBR and PS as the synth makes them)"""
    rng = np.random.default_rng(seed)
    n = WIN_STREAMS
    frames = list(synth.he_stream(rng, cfg, n, WIN_STEPS, hdr, ps_mode=ps_mode, hdr_choice=np.arange(n) % len(hdr),
                                  coupling=0.5 if cfg == pkg.CFG_HEV1 else 0.0))
    own = np.random.default_rng([seed, 101])
    ncore = 2 if cfg == pkg.CFG_HEV1 else 1
    per_ch = [window_ics(pkg, n, WIN_STEPS, c) for c in range(ncore)]
    for t, fr in enumerate(frames):
        fr["ics"] = np.ascontiguousarray(np.stack([p[t] for p in per_ch], axis=1))
        fr["coeffs"] = _window_coeffs(synth, own, fr["ics"], 400)
    return frames


# ---------------------------------------------------------------------------
# what a run holds (tests/test_grid_reach.py: the profiles' floors, and the plain synth's baseline)
# ---------------------------------------------------------------------------
def sbr_counts(frames, hdr, ncore, widest=None):
    """Counter over the grids of a run (started frames; the second channel of a coupled pair repeats the first)."""
    from collections import Counter
    c = Counter()
    for step in frames:
        for s in range(step["sbr"].shape[0]):
            fr = step["sbr"][s]
            if not fr["start"]:
                continue
            for k in range(ncore):
                if k and fr["bs_coupling"]:
                    continue
                ch = fr["ch"][k]
                L = int(ch["bs_num_env"])
                t = [int(x) for x in ch["t_env"][: L + 1]]
                c["grids"] += 1
                c["L", L] += 1
                c["L5_widest"] += L == 5 and widest is not None and int(fr["hdr"]) == widest
                c["first_one_slot"] += t[1] - t[0] == 1
                c["last_one_slot"] += t[L] - t[L - 1] == 1
                c["one_slot_pairs"] += sum(t[i + 2] - t[i] == 2 for i in range(L - 1))
                c["longest"] += t == [0, 19]
                c["shortest"] += t == [3, 16]
                seam = t[0] - max(int(ch["t_env_num_env_old"]) - 16, 0)
                if seam:
                    c["gap" if seam > 0 else "overlap", abs(seam)] += 1
                    c["seam_reset" if fr["reset"] else "seam_no_reset"] += 1
                    c["seam_smoothing" if not hdr[int(fr["hdr"])]["bs_smoothing_mode"] else "seam_plain"] += 1
                if "pointer" in step:
                    c["pointer", int(step["pointer"][s, k])] += 1
                c["t_q1_no_border"] += L > 1 and int(ch["t_q"][1]) not in t
                c["e_a", int(ch["e_a"][0]), int(ch["e_a"][1])] += 1
                c["t_old_below_16"] += int(ch["t_env_num_env_old"]) < 16
                c["steps_6_8"] += any(t[i + 1] - t[i] in (6, 8) for i in range(L)) and L not in (1, 2)
    return c


def ps_counts(frames):
    from collections import Counter
    c = Counter()
    for step in frames:
        for p in step["ps"]:
            if not p["start"]:
                continue
            E = int(p["num_env"])
            b = tuple(int(x) for x in p["border_position"][: E + 1])
            c["frames"] += 1
            c["E", E] += 1
            c["borders", b] += 1
            c["aligned_uneven"] += list(b) in [list(x) for x in ALIGNED_UNEVEN]
            c["first_one_slot"] += b[1] - b[0] == 1
            c["last_one_slot"] += b[E] - b[E - 1] == 1
            c["num_env_old", int(p["num_env_old"])] += 1
            c["layout_switch"] += int(p["is34bands"]) != int(p["is34bands_old"])
            c["ipdopd", int(p["enable_ipdopd"])] += 1
    return c


def window_combinations(ics_steps, channel):
    """the (ws, ws_prev, kb, kb_prev) combinations one channel of a run takes; ics_steps: [steps] of ics [n][ch]"""
    return {(int(i["window_sequence"][0]), int(i["window_sequence"][1]), int(i["use_kb_window"][0]),
             int(i["use_kb_window"][1])) for ics in ics_steps for i in ics[:, channel]}

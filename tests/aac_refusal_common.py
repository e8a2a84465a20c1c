"""Shared by tests/test_aac_parse_refusal_state.py and tests/golden/make_aac_refusal_states.py: the refusal exits of the
host AAC parser with the status each has, and the replay of one fixture case."""
import hashlib

import numpy as np

DATA, OVERREAD, UNSUPPORTED = -1, -2, -3
# exit -> (status, the refusal is the reference's own); written down from the reference's text, not from a run
READER_EXITS = {
    "reserved_bit": (DATA, 1), "prediction_in_aac_lc": (DATA, 1), "reset_group_0": (DATA, 1), "reset_group_31": (DATA, 1),
    "max_sfb_above_num_swb": (DATA, 1), "band_type_12": (DATA, 1), "section_past_max_sfb": (DATA, 1),
    "escape_run_overreads": (OVERREAD, 1), "gain_offset_out_of_range": (DATA, 1), "noise_offset_out_of_range": (DATA, 1),
    "intensity_offset_out_of_range": (DATA, 1), "pulse_in_eight_short": (DATA, 1), "pulse_band_above_num_swb": (DATA, 1),
    "pulse_position_above_1023": (DATA, 1), "tns_order_above_maximum": (DATA, 1), "gain_control": (UNSUPPORTED, 1),
    "escape_prefix_of_9_ones": (DATA, 1), "overread_inside_the_spectrum": (OVERREAD, 0), "ms_present_3": (DATA, 1),
}
LOOP_EXITS = {
    "dse_longer_than_the_unit": (OVERREAD, 0), "fill_element_longer_than_the_unit": (OVERREAD, 1),
    "sbr_payload_before_the_first_channel_element": (DATA, 0), "second_sbr_payload": (UNSUPPORTED, 0),
    "fewer_than_3_bits_left": (OVERREAD, 1),
}
READER_PLACES = {"sce", "cpe_ch0", "cpe_ch1", "cpe_common_ch0", "cpe_common_ch1", "layout_second_element"}
LOOP_PLACES = {"sce", "cpe", "layout_second_element"}


def replay(pkg, case):
    """The case's units through the host parser of pkg.lib(): what the generator stores and the test compares."""
    cfg = pkg.AacConfig()
    cfg.object_type, cfg.sampling_index, cfg.sample_rate, cfg.chan_config = case["aot"], case["si"], 48000, case["chan_config"]
    if case["layout"]:
        rc, lay = pkg.aac_layout_default(case["chan_config"])
        assert rc == 0
        st = np.zeros(int(lay[0]["n_elements"]), pkg.AAC_STREAM_DT)
        keys = ("tools", "coeffs", "ics", "elem")
        parse = lambda au: pkg.aac_parse_frame_layout(cfg, lay, st, au)
        rows = lambda: st.tobytes().hex() + lay.tobytes().hex()
    else:
        st = np.zeros(1, pkg.AAC_STREAM_DT)
        keys = ("tools", "coeffs", "ics")
        parse = lambda au: pkg.aac_parse_frame_ex(cfg, st, au, 2, with_cce=False)
        rows = lambda: st.tobytes().hex()

    def run(unit):
        r, out = parse(bytes.fromhex(unit))
        return r, [int(x) for x in out["info"][0].tolist()], hashlib.sha256(b"".join(out[k].tobytes() for k in keys)).hexdigest()

    for unit in case["setup"]:
        assert run(unit)[0] == 0
    got = dict(st_before=rows())
    got["status"], got["info"], got["sha256"] = run(case["unit"])
    got["st_after"] = rows()
    got["next_status"], got["next_info"], got["next_sha256"] = run(case["next"])
    got["st_next"] = rows()
    return got

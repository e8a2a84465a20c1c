"""What heaac_sbr_parse_payload leaves behind a payload it refuses (CPU).  The host parser does not defer: the state a
Parametric Stereo error leaves in the stream row is read by later frames (num_env_old, the rows time deltas continue
from, is34bands), and a refused element must leave both channels and bs_coupling as they were.  test_sbr_parse.py looks
at `start` only and the walk-against-host comparisons of test_sbr_core.py skip the units the walk gives up, so the
exits are pinned here, byte for byte, against tests/golden/sbr_error_states.json.

The fixture was minted by tests/golden/make_sbr_error_states.py against a build of commit 63469a7, the last one in which
csrc/sbr_parse.c held readers of its own -- not against the tree under test.  Each case: a stream of the bit writer two
good frames in (plus a set-up frame where the case needs one), then one payload: one per exit of the PS reader (sc_ps
of csrc/sbr_core.h), each of test_sbr_parse.BAD_GRIDS in an SCE and in the second channel of an uncoupled CPE, an
envelope value pushed above 255, a truncated unit.  Stored are the status, the HeaacSbrParseInfo, both records, the state
row as its difference from the row in front of the unit, and the status and records of one good writer frame parsed
after it.  The exit "a prefix that is no code" has no case: the twenty code books are complete and the bit reader
yields zeros past the end of a unit, so no payload reaches it (the generator checks the Kraft sums)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "sbr_error_states.json")) as f:
    CASES = json.load(f)["cases"]

PS_EXITS = {"ps_reserved_iid_mode", "ps_reserved_icc_mode", "ps_iid_value_out_of_range", "ps_icc_value_out_of_range",
            "ps_extensions_past_their_count", "ps_borders_not_ascending", "ps_borrowed_value_outside_the_quantiser",
            "ps_longer_than_its_extension"}


def test_the_fixture_holds_every_case():
    names = {c["name"] for c in CASES}
    assert PS_EXITS <= names
    for where in ("an_sce", "the_second_channel_of_a_cpe"):
        assert {"bad_grid_%d_in_%s" % (g, where) for g in range(4)} <= names
    assert {"envelope_value_above_255", "truncated_unit"} <= names
    by = {c["name"]: c for c in CASES}
    assert by["ps_longer_than_its_extension"]["expect"]["status"] == -2                  # HEAAC_PARSE_ERR_OVERREAD
    assert all(by[n]["expect"]["status"] == -1 for n in PS_EXITS - {"ps_longer_than_its_extension"})


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_state_and_records_after_a_refused_payload(pkg, case):
    channels, allow_ps = case["channels"], bool(case["allow_ps"])
    tab = pkg.SbrHeaderTable(8)
    st = pkg.sbr_streams(1)

    def parse(payload_hex):
        r, sbr, ps, info = pkg.sbr_parse_payload(st[0], tab, 24000, bytes.fromhex(payload_hex), channels, allow_ps)
        return r, sbr.tobytes().hex(), ps.tobytes().hex(), [int(info[k]) for k in ("sbr_bits", "header", "ps_present", "ps_status")]

    for payload in case["setup"]:
        assert parse(payload)[0] == 0
    want = st[0].copy()
    for at, data in case["expect"]["state_diff"]:
        data = np.frombuffer(bytes.fromhex(data), np.uint8)
        want[at:at + len(data)] = data
    exp = case["expect"]
    r, sbr, ps, info = parse(case["unit"])
    assert (r, info) == (exp["status"], exp["info"])
    assert sbr == exp["sbr"], "sbr record"
    assert ps == exp["ps"], "ps record"
    moved = np.flatnonzero(st[0] != want)
    assert moved.size == 0, ("state row", moved[:16].tolist(), st[0][moved[:16]].tolist(), want[moved[:16]].tolist())
    nxt = case["next"]
    r, sbr, ps, _ = parse(nxt["payload"])
    assert r == nxt["status"]
    assert sbr == nxt["sbr"], "sbr record of the next frame"
    assert ps == nxt["ps"], "ps record of the next frame"

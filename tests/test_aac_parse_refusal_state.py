"""What the host AAC parser leaves behind an access unit it refuses (CPU).  A refusal is observable: the status, the
HEAAC_REFUSED_* flags, the window history the reference's decoders had moved or cleared by then, the records the
spectral tools are to run on.  The device walk gives such a unit up and the walk-against-host comparisons of
test_parse_core.py skip it, so the exits are pinned here against tests/golden/aac_refusal_states.json.

The fixture was minted by tests/golden/make_aac_refusal_states.py against a build of commit 0e82445, the last one in
which csrc/aac_parse.c held readers of its own -- not against the tree under test.  Each case: a stream one good unit
in, then one crafted unit that takes one refusal exit of the readers of csrc/parse_core.h or of the element loops of
csrc/aac_parse.c -- in an SCE, in either channel of a CPE with and without a common window, in the second element of a
3.0 layout -- then one good unit.  Stored are the status, the HeaacAacFrameInfo, the stream rows before and after, a
SHA-256 over the tools records, coefficient rows, window records and element infos, and the same for the good unit
parsed after it.  The exit "a prefix that is no code of the book" has no case: the twelve code books are complete, so
every prefix is a code (the generator checks the Kraft sums)."""
import json
import os

import pytest

from aac_refusal_common import LOOP_EXITS, LOOP_PLACES, READER_EXITS, READER_PLACES, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "aac_refusal_states.json")) as f:
    CASES = json.load(f)["cases"]

def test_the_fixture_holds_every_exit_in_every_place():
    seen = {}
    for c in CASES:
        seen.setdefault(c["exit"], set()).add(c["place"])
        want = {**READER_EXITS, **LOOP_EXITS}[c["exit"]]
        assert (c["expect"]["status"], c["expect"]["info"][8] & 1) == want, c["name"]
        assert c["expect"]["next_status"] == 0, c["name"]
    for e in READER_EXITS:
        if e == "ms_present_3":
            assert seen[e] == {"cpe_common_head", "layout_second_element"}
        elif e in ("reserved_bit", "prediction_in_aac_lc", "reset_group_0", "reset_group_31", "max_sfb_above_num_swb"):
            # inside ics_info: with a common window the pair has one, at its head
            assert seen[e] == (READER_PLACES - {"cpe_common_ch0", "cpe_common_ch1"}) | {"cpe_common_head"}, e
        else:
            assert seen[e] == READER_PLACES, e
    for e in LOOP_EXITS:
        assert seen[e] == LOOP_PLACES, e
    # both classes of what a refusal leaves are there: history moved or cleared, and work left for the spectral tools
    assert any(c["expect"]["info"][8] == 3 for c in CASES) and any(c["expect"]["info"][8] == 1 for c in CASES)
    assert any(c["expect"]["st_after"] != c["expect"]["st_before"] for c in CASES)
    assert any(c["aot"] == 1 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_state_and_records_after_a_refused_unit(pkg, case):
    got, exp = replay(pkg, case), case["expect"]
    for k in ("st_before", "status", "info", "st_after", "sha256", "next_status", "next_info", "st_next", "next_sha256"):
        assert got[k] == exp[k], k

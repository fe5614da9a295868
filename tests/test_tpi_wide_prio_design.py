"""The issue-priority ladder of tpi_ring_wide_kernel<67> in the compiled code (no GPU needed).

tools/valu_bound.py wide cross-compiles the kernel, asserts the ladder's shape and reports it; the same source built with
-DWIDE_PRIO=0 must give the chain waves the same work.

The two chain loops are NOT identical line for line once the s_setprio lines are removed: with the ladder the compiler
allocates a few registers differently and orders a handful of DPP adds differently around the switches (266 differing
diff lines of 1324).  So, as the fallback, the counts are compared: the vector instructions by opcode and the ds_read
instructions are equal.  The s_nop count is not: 16 without the ladder, 15 with it.  The padding in this loop is the wait
states between a vector write and the DPP read of that register; an s_setprio is an instruction issued by the wave like
any other and counts as such a wait state, and one switch falls where an `s_nop 0` stood.  Placing the switches elsewhere
(before or behind the fetch, behind the scheduling barrier, fenced by barriers of their own; the first raise before the lead
fetches) gave 15 every time.  What is asserted is therefore that the ladder build has no more s_nop than the plain build
and at most one fewer per switch inside the sweep; both counts are printed."""
import json
import os
import subprocess
import sys
from collections import Counter

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


@pytest.fixture(scope="module")
def report():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "valu_bound.py"), "wide"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout)


def test_ladder_shape(report):
    pair = report["row_pair_instructions"]
    lad = pair["priority_ladder"]
    assert pair["valu"] == 811 and pair["vmcnt_waits"] == 0 and pair["ds_read_b64"] == 165
    assert lad["levels"] == [3, 2, 1, 0] and lad["last_level_before_first_store"] is True
    total = pair["valu"]
    assert sum(lad["valu_by_level"]) + lad["valu_outside_the_ladder"] == total
    assert max(lad["valu_by_level"]) <= lad["bounds"]["level_share"] * total
    assert lad["valu_by_level"][-1] <= lad["bounds"]["last_level_share"] * total
    assert lad["bounds"] == {"level_share": 0.40, "last_level_share": 0.20}
    stg = report["staging_phase_loop"]["lean_path"]
    assert stg["priority"] == {"levels": [3, 0], "raised_before_first_convert": True, "lowered_before_barrier": True}
    assert stg["valu"] == 146 and stg["valu_by_op"]["v_fract_f32_e32"] == 32


def test_chain_loop_is_the_plain_builds_but_for_the_switches():
    import valu_bound as vb

    plain = vb.chain_phase_loop(vb.wide_asm(["-DWIDE_PRIO=0"]))
    ladder = vb.chain_phase_loop(vb.wide_asm())
    assert not any(x.startswith("s_setprio") for x in plain)
    switches = sum(x.startswith("s_setprio") for x in ladder)
    assert switches == 4
    ops_p, ops_l = Counter(x.split()[0] for x in plain), Counter(x.split()[0] for x in ladder)
    for pick in ("v_", "ds_read"):
        assert {k: v for k, v in ops_p.items() if k.startswith(pick)} == {k: v for k, v in ops_l.items() if k.startswith(pick)}, pick
    print("s_nop: plain", ops_p["s_nop"], "ladder", ops_l["s_nop"])
    assert ops_p["s_nop"] - (switches - 1) <= ops_l["s_nop"] <= ops_p["s_nop"]
    assert len(ladder) - switches <= len(plain)

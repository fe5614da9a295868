"""The strip width of tpi_ring_wide_kernel<67> and its chain waves' phase boundary in the compiled code (DESIGN.md K1
round 14; no GPU needed).

tools/valu_bound.py wide cross-compiles the kernel and reports (phase_boundary) the chain waves' way from the phase barrier
to the sweep, for the loop that ships and for the lab switch -DWIDE_BOUNDARY=1.  Round 14 built that switch, measured it
and did not keep it in the product (the bench step did not follow the counters), so:

  * what ships has 316 valid columns a strip, read from the compiled unit (WGeo<67>::TILE_W), round 13's boundary - no
    fetch in front of the barrier - and the counts tests/test_tpi_wide_prio_design.py pins;
  * the lab build stays what was measured:
    (a) the reads of the NEXT phase's lead fetches - three ds_read_b64 a prefix row - between the phase's last output
        store and s_barrier, with no s_waitcnt lgkmcnt(0) between them and the barrier;
    (b) on the hot path from s_barrier to the sweep's first `s_setprio 3` no s_mul_hi*, no s_mulk_i32, no v_readlane;
    (c) fewer instructions on the hot path from s_barrier to the sweep's first vector subtract than in the shipped loop,
        counted by the same walk;
    and the sweep's 165 reads."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "valu_bound.py"), "wide"], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout)


def test_what_ships(report):
    assert report["valid_columns_per_wave_row"] == 316
    pair = report["row_pair_instructions"]
    assert pair["valu"] == 811 and pair["ds_read_b64"] == 165 and pair["vmcnt_waits"] == 0
    assert pair["priority_ladder"]["levels"] == [3, 2, 1, 0]
    assert pair["phase_boundary"]["lead_reads_between_last_store_and_barrier"] == 0
    lean = report["staging_phase_loop"]["lean_path"]
    assert lean["valu"] == 146 and lean["valu_by_op"]["v_fract_f32_e32"] == 32 and lean["priority"]["levels"] == [3, 0]


def test_lab_lead_fetches_stand_in_front_of_the_barrier(report):
    lab = report["row_pair_instructions"]["phase_boundary"]["lab_WIDE_BOUNDARY_1"]
    assert lab["lead_rows"] == 7, "67 px, WIDE_LEAD = 2: four rows of the first fetch, three of the second"
    assert lab["lead_reads_between_last_store_and_barrier"] == 3 * lab["lead_rows"]
    assert lab["lgkmcnt0_wait_between_lead_reads_and_barrier"] is False
    assert lab["ds_read_b64"] == 165


def test_lab_no_multiplication_or_reload_behind_the_barrier(report):
    b = report["row_pair_instructions"]["phase_boundary"]
    assert b["lab_WIDE_BOUNDARY_1"]["multiplies_and_readlanes_before_the_sweep"] == []
    assert b["multiplies_and_readlanes_before_the_sweep"], "the shipped path holds the % R chain: the walk must find it"


def test_lab_hot_path_behind_the_barrier_is_shorter(report):
    b = report["row_pair_instructions"]["phase_boundary"]
    now, shipped = b["lab_WIDE_BOUNDARY_1"]["hot_path_barrier_to_first_subtract"], b["hot_path_barrier_to_first_subtract"]
    print(f"barrier to first subtract: lab {now} instructions, shipped {shipped}")
    assert 0 < now < shipped

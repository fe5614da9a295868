#!/usr/bin/env python3
"""Vector-ALU bound of the headline kernel (tpi_march_kernel<67, 60, 12>) from its own instruction stream.

What bounds TPI at 67 px is vector-ALU issue, not HBM.  This tool makes that a number the bench
line can carry: it compiles the kernel from the product's headers (tools/ubench/tpi_lab.hip, device code only),
finds the row loop in the ISA (the loop that holds the 42 ds_read_b128 of a 67-px chain), counts its vector
instructions by issue class and prices them with the issue costs measured on the GPU
(profiles/r02_valu_mix_rate.txt, profiles/r03_valu_mix2_rate.txt: 1.05 ns per wave-instruction and SIMD for plain
VOP1 / VOP2 integer and float operations, 1.87 ns for every DPP form, v_add3_u32, VOP3-only integer operations,
converts and float64).  The instructions outside the row loop (staging, tile bookkeeping) come from the launch's
SQ_INSTS_VALU counter minus the row loop's share and are priced at the kernel's overall mix.

    python tools/valu_bound.py [SQ_INSTS_VALU per launch, default from profiles/r06_tpi67_pmc_summary.txt] > profiles/r06_tpi67_valu_bound.json
    python tools/valu_bound.py std [SQ_INSTS_VALU per launch, default from profiles/r06_std67_pmc_summary.txt] > profiles/r06_std67_valu_bound.json

    python tools/valu_bound.py wide > profiles/r14_tpi67_wide_valu_count.json

wide: one output row of tpi_ring_wide_kernel<67> (csrc/disc_ring_wide_impl.hpp: 6 columns per lane, 316 valid columns a
row, the number read from the compiled unit) counted the same way from a device-only compile of the product's header, and set against the marching kernel's
row loop per VALID output column: offline, before any GPU time.  A chain wave sums its two rows of a phase in one sweep
(55 distinct prefix rows of three ds_read_b64 for the pair), so the count is that of the chain waves' phase loop - the
sweep, the finalisation and the stores of both rows, the barrier - and an output row is half of it.  Vector adds whose
result is a ds_read address are counted as their own class.  The staging waves' phase loop is reported beside it
(staging_phase_loop): every instruction the loop holds, and the way round it that an interior batch takes (the lean path of
stage_batch and load_batch) - instructions, VALU by opcode, scalar instructions, branches, the VALU's price.  The issue
priorities (WIDE_PRIO) are part of the count: the chain loop's s_setprio levels and the VALU each covers, the staging
loop's raise and drop (priority_ladder, priority), with the ladder's shape asserted.  The chain waves' way from the phase
barrier to the sweep's first subtract is walked and counted (phase_boundary), for the loop that ships and for the lab switch
-DWIDE_BOUNDARY=1 (round 14: the next phase's lead fetches in front of the barrier; measured, not kept), whose shape is asserted.

std (round 4): the same for std_ring_kernel<67, false> - its phase loop (one output row of 256 pixels per wave and
phase: two chains, the staging share of the wave, the finalisation) priced by issue class; the scalar instructions of
the loop are counted next to it (they issue beside the vector ones of the other waves of the SIMD).
"""
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NS_PLAIN, NS_HALF = 1.05, 1.87          # ns per wave-instruction and SIMD (16 waves per CU, wall clock)
NY = NX = 32768
SIZE, TH, TILE_W = 67, 60, 184
KERNEL = "tpi_march_kernelILi67ELi60ELi12ELb1ELb1ELb1"
STD_KERNEL = "std_ring_kernelILi67ELb0ELi0"
SUFFIX = "EEEvNS0_8WaveArgsEiiNS0_7PartRunE:"   # (WaveArgs, int, int, PartRun): the ordinary (one-part) kernels


def half_rate(op):
    return ("_dpp" in op or "add3" in op or "f64" in op or op.startswith("v_cvt") or op.startswith("v_mad") or
            op.startswith("v_mul_lo") or op.startswith("v_mul_hi") or op.startswith("v_lshl_add") or
            op.startswith("v_bfe") or op.startswith("v_perm") or op.startswith("v_cndmask") and op.endswith("e64") or
            op.startswith("v_cmp") or op.startswith("v_max3") or op.startswith("v_min3") or op.startswith("v_readlane") or
            op.startswith("v_writelane") or
            # measured in round 12 (tools/ubench/valu_mix3.hip, profiles/r12_valu_mix3_rate.txt): 1.87 / 1.89 ns at 16 waves per CU
            op.startswith("v_fract") or op.startswith("v_or3"))


WIDE_KERNEL = "tpi_ring_wide_kernelILi67"
WIDE_SRC = """#include "disc_wave_impl.hpp"
namespace topo { int wide_probe(const Block& b, float* t) { return launch_ring_wide<67>(b, t, 60, 184); }
extern "C" __device__ __attribute__((used)) const int wide_probe_tile_w = WGeo<67>::TILE_W;
extern "C" __device__ __attribute__((used)) const int wide_probe_lead_rows = WPair<67, WideCfg<67>::GR>::lead_rows(WIDE_LEAD); }
"""


def loop_lines(txt, kernel, pick):
    """The instruction lines of the smallest loop of `kernel` (mangled name prefix) whose mnemonics `pick(ops)` accepts."""
    start = txt.index(kernel + SUFFIX)
    lines = txt[start:txt.index("s_endpgm", start)].split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = None
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.search(r"s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            a = labels[m.group(1)]
            o = [x.strip() for x in lines[a:i + 1]
                 if x.strip() and not x.strip().startswith((".", ";", "//")) and not x.strip().endswith(":")]
            if pick([x.split()[0] for x in o]) and (best is None or len(o) < len(best)):
                best = o
    return best


def loop_ops(txt, kernel, pick):
    """The mnemonics of loop_lines."""
    o = loop_lines(txt, kernel, pick)
    return None if o is None else [x.split()[0] for x in o]


def address_adds(lines):
    """Vector adds whose result register is the address of a ds_read before it is written again."""
    n = 0
    for i, x in enumerate(lines):
        if not x.startswith("v_add_u32"):
            continue
        dst = x.split()[1].rstrip(",")
        for y in lines[i + 1:]:
            f = y.replace(",", " ").split()
            if f[0].startswith("ds_read") and len(f) > 2 and f[2] == dst:
                n += 1
                break
            if f[0].startswith("v_") and len(f) > 1 and f[1] == dst:
                break
    return n


def price(o):
    valu = [x for x in o if x.startswith("v_")]
    kinds = Counter()
    for x in valu:
        kinds["dpp" if "_dpp" in x else "add3" if "add3" in x else "f64_or_convert" if ("f64" in x or x.startswith("v_cvt")) else
              "other_half_rate" if half_rate(x) else "plain"] += 1
    mix = Counter("half" if half_rate(x) else "plain" for x in valu)
    return valu, kinds, mix["plain"] * NS_PLAIN + mix["half"] * NS_HALF


def blocks_of(lines):
    """Basic blocks of a loop body (instruction lines and labels, in order): [label or None, [instructions]]."""
    out = [[None, []]]
    for x in lines:
        x = x.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", x)
        if m:
            out.append([m.group(1), []])
        elif x and not x.startswith((".", ";", "//")):
            out[-1][1].append(x)
            if x.startswith(("s_cbranch", "s_branch")):
                out.append([None, []])
    return [b for b in out if b[0] or b[1]]


def rows_written(mn):
    """Ring rows a list of mnemonics writes: a ds_write2(st64)_b64 carries two."""
    return mn.count("ds_write_b64") + 2 * sum(1 for x in mn if x.startswith("ds_write2") and x.endswith("_b64"))


def staging_loop(txt):
    """The staging waves' phase loop of the wide kernel: the smallest loop that loads a batch (16 global_load_dwordx2) and
    writes it (16 ds_write_b64), meets the phase barrier and has no float64 (the run's prologue stages batches in a loop of its
    own, with no barrier in it).  Returns (all its instructions, the shortest way round it that still
    loads and writes a batch: the lean path of an interior batch, with no guard copies and no phase that is not computed)."""
    start = txt.index(WIDE_KERNEL + SUFFIX)
    lines = txt[start:txt.index("s_endpgm", start)].split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = None
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.search(r"s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            body = lines[labels[m.group(1)]:i + 1]
            mn = [x.split()[0] for x in body if x.strip() and not x.strip().startswith((".", ";", "//")) and not x.strip().endswith(":")]
            if (mn.count("global_load_dwordx2") >= 16 and rows_written(mn) >= 16 and "s_barrier" in mn
                    and not any("f64" in x for x in mn) and (best is None or len(body) < len(best))):
                best = body
    assert best is not None, "no staging phase loop found"
    bl = blocks_of(best)
    at = {b[0]: k for k, b in enumerate(bl) if b[0]}
    shortest = [None]

    def walk(k, path, seen):
        while True:
            if k >= len(bl):
                return
            path = path + bl[k][1]
            seen = seen | {k}
            last = bl[k][1][-1] if bl[k][1] else ""
            tgt = (last.split()[1] if last.startswith(("s_cbranch", "s_branch")) else None)
            if k == len(bl) - 1:  # the back edge
                mn = [x.split()[0] for x in path]
                if mn.count("global_load_dwordx2") >= 16 and rows_written(mn) >= 16 and (shortest[0] is None or len(path) < len(shortest[0])):
                    shortest[0] = path
                return
            if tgt is not None and tgt in at and at[tgt] > k and at[tgt] not in seen:
                walk(at[tgt], path, seen)
            if last.startswith("s_branch"):
                return
            k += 1

    walk(0, [], frozenset())
    assert shortest[0] is not None, "no way round the staging loop that loads and writes a batch"
    return [x for b in bl for x in b[1]], shortest[0]


def staging_report(lines):
    mn = [x.split()[0] for x in lines]
    valu, kinds, ns = price(mn)
    return {"instructions": len(mn), "valu": len(valu), "valu_half_rate": sum(1 for x in valu if half_rate(x)),
            "valu_by_op": dict(Counter(valu).most_common()), "salu": sum(1 for x in mn if x.startswith("s_")),
            "salu_by_op": dict(Counter(x for x in mn if x.startswith("s_")).most_common()),
            "branches": sum(1 for x in mn if x.startswith(("s_cbranch", "s_branch"))),
            "global_load_dwordx2": mn.count("global_load_dwordx2"), "ring_rows_written": rows_written(mn),
            "valu_ns": round(ns, 1)}


def wide_asm(extra=()):
    """The ISA of a device-only compile of the wide kernel from the product's header (`extra`: further compiler flags)."""
    csrc = os.path.join(REPO, "topo_descriptors_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        src, asm = os.path.join(tmp, "wide.hip"), os.path.join(tmp, "wide.s")
        open(src, "w").write(WIDE_SRC)
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I", csrc, "-I", os.path.join(REPO, "include"), *extra, src, "-o", asm], check=True, stderr=subprocess.DEVNULL)
        return open(asm).read()


def chain_phase_loop(txt):
    """The chain waves' phase loop: ONE sweep over the wave's row pair (55 distinct prefix rows of the pair's 84, three
    ds_read_b64 each), the float64 finalisation and the stores of both rows, the barrier."""
    return loop_lines(txt, WIDE_KERNEL, lambda o: sum(x == "ds_read_b64" for x in o) >= 3 * 42 and any("f64" in x for x in o))


def probe_constant(txt, name):
    """A constant of the compiled unit (WIDE_SRC): what the headers themselves say."""
    return int(re.search(r"^%s:\s*\n\s*\.long\s+(\d+)" % name, txt, re.M).group(1))


def chain_loop_blocks(txt):
    """The chain waves' phase loop (chain_phase_loop) as basic blocks, labels kept: [label or None, [instructions]]."""
    start = txt.index(WIDE_KERNEL + SUFFIX)
    lines = txt[start:txt.index("s_endpgm", start)].split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = None
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.search(r"s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            body = lines[labels[m.group(1)]:i + 1]
            mn = [x.split()[0] for x in body if x.strip() and not x.strip().startswith((".", ";", "//")) and not x.strip().endswith(":")]
            if sum(x == "ds_read_b64" for x in mn) >= 3 * 42 and any("f64" in x for x in mn) and (best is None or i - labels[m.group(1)] < best[1] - best[0]):
                best = (labels[m.group(1)], i)
    assert best is not None, "no chain phase loop found"
    # (the loop's layout may put blocks of it in front of the label its last branch returns to: taken in with the body)
    a, b = best
    while True:
        tg = [labels[t] for l in lines[a:b + 1] for t in re.findall(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l) if t in labels and labels[t] < a]
        if not tg:
            break
        a = min(tg)
    return blocks_of(lines[a:b + 1])


def boundary_path(bl):
    """The hot path of a chain wave from the phase barrier to the sweep: the way through the loop's blocks (the back edge
    included) with the fewest instructions from behind s_barrier to the first vector subtract behind `s_setprio 3`.
    Returns the instructions on it, the barrier and the subtract excluded."""
    at = {b[0]: k for k, b in enumerate(bl) if b[0]}
    bar = [(k, i) for k, b in enumerate(bl) for i, x in enumerate(b[1]) if x.startswith("s_barrier")]
    assert len(bar) == 1, f"chain loop: {len(bar)} barriers"

    def sweep_start(ins, lo=0):
        """Index of the first v_sub_u32 behind an `s_setprio 3` among ins[lo:], or None."""
        raised = False
        for i in range(lo, len(ins)):
            raised = raised or ins[i].split()[:2] == ["s_setprio", "3"]
            if raised and ins[i].startswith("v_sub_u32"):
                return i
        return None

    def succ(k):
        last = bl[k][1][-1] if bl[k][1] else ""
        out = []
        if last.startswith(("s_cbranch", "s_branch")):
            tgt = last.split()[1]
            if tgt in at:
                out.append(at[tgt])
        if not last.startswith("s_branch") and k + 1 < len(bl):
            out.append(k + 1)
        return out

    k0, i0 = bar[0]
    end = sweep_start(bl[k0][1], i0 + 1)
    if end is not None:
        return bl[k0][1][i0 + 1:end]
    # Dijkstra over the blocks: cost = instructions issued
    import heapq
    heap = [(len(bl[k0][1]) - i0 - 1, n, bl[k0][1][i0 + 1:]) for n in succ(k0)]
    heapq.heapify(heap)
    done = set()
    while heap:
        cost, k, path = heapq.heappop(heap)
        if k in done:
            continue
        done.add(k)
        end = sweep_start(bl[k][1])
        if end is not None:
            return path + bl[k][1][:end]
        for n in succ(k):
            if n not in done:
                heapq.heappush(heap, (cost + len(bl[k][1]), n, path + bl[k][1]))
    raise AssertionError("chain loop: no way from the barrier to the sweep")


def boundary_report(txt, lead_rows):
    """The chain waves' phase boundary (WIDE_BOUNDARY): the lead fetches in front of the barrier, the hot path behind it."""
    bl = chain_loop_blocks(txt)
    ph = [x for b in bl for x in b[1]]
    prio = [i for i, x in enumerate(ph) if x.startswith("s_setprio")]
    stores = [i for i, x in enumerate(ph) if x.startswith("global_store_dwordx2") and i > prio[0]]
    bar = [i for i, x in enumerate(ph) if x.startswith("s_barrier")][0]
    # (in the loop's order: what follows the last output store, round the back edge if the barrier stands in front of it)
    between = ph[stores[-1] + 1:bar] if bar > stores[-1] else ph[stores[-1] + 1:] + ph[:bar]
    reads = [i for i, x in enumerate(between) if x.startswith("ds_read_b64")]
    wait0 = bool(reads) and any(x.startswith("s_waitcnt") and "lgkmcnt(0)" in x for x in between[reads[0]:])
    path = boundary_path(bl)
    mn = [x.split()[0] for x in path]
    to_prio = mn[:max(i for i, x in enumerate(path) if x.split()[:2] == ["s_setprio", "3"])] if "s_setprio" in mn else mn
    return {"lead_rows": lead_rows, "lead_reads_between_last_store_and_barrier": len(reads),
            "lgkmcnt0_wait_between_lead_reads_and_barrier": wait0,
            "hot_path_barrier_to_first_subtract": len(path),
            "hot_path_salu": sum(x.startswith("s_") for x in mn), "hot_path_valu": sum(x.startswith("v_") for x in mn),
            "hot_path_ds_reads": sum(x.startswith("ds_read") for x in mn),
            "hot_path_waits": [x for x in path if x.startswith("s_waitcnt")],
            "multiplies_and_readlanes_before_the_sweep": [x for x in to_prio if x.startswith(("s_mul_hi", "s_mulk_i32", "v_readlane"))]}


# The chain waves' priority ladder (WIDE_PRIO): the wave behind catches up while the wave ahead sits a level lower, so the
# lag between a SIMD's two chain waves is bounded by a level's width - no level may hold more than LEVEL_SHARE of the loop's
# VALU - and on the last level, where both are at 0 and age alone decides, the younger wave runs on alone once the older is
# through: at most LAST_SHARE.
LEVEL_SHARE, LAST_SHARE = 0.40, 0.20


def ladder_report(ph):
    """The s_setprio levels of the chain waves' phase loop and the VALU each covers (asserts the ladder's shape)."""
    at = [(i, int(x.split()[1])) for i, x in enumerate(ph) if x.startswith("s_setprio")]
    levels = [l for _, l in at]
    assert levels == sorted(set(levels), reverse=True) and len(levels) >= 2 and levels[0] == 3, f"chain loop: the levels {levels} do not descend from 3"
    # (the output stores: the loop's layout puts the phase's bookkeeping, the tile map's stores among it, in front of the sweep)
    stores = [i for i, x in enumerate(ph) if x.startswith("global_store_dwordx2") and i > at[0][0]]
    assert levels[-1] == 0 and stores and at[-1][0] < stores[0], "chain loop: the wave is not back at 0 before its first output store"
    assert not any(x.startswith(("s_cbranch", "s_branch")) for x in ph[at[0][0]:at[-1][0]]), "chain loop: a branch inside the sweep"
    ends = [i for i, _ in at[1:]] + [len(ph)]
    segs = [[x.split()[0] for x in ph[a:b] if x.startswith("v_")] for (a, _), b in zip(at, ends)]
    valu = [len(v) for v in segs]
    total = sum(x.startswith("v_") for x in ph)
    shares = [round(v / total, 3) for v in valu]
    assert max(shares) <= LEVEL_SHARE, f"chain loop: a level holds {max(shares)} of the VALU (at most {LEVEL_SHARE})"
    assert shares[-1] <= LAST_SHARE, f"chain loop: the last level holds {shares[-1]} of the VALU (at most {LAST_SHARE})"
    return {"levels": levels, "valu_by_level": valu, "ns_by_level": [round(price(v)[2], 1) for v in segs], "share_by_level": shares,
            "valu_outside_the_ladder": total - sum(valu), "bounds": {"level_share": LEVEL_SHARE, "last_level_share": LAST_SHARE},
            "last_level_before_first_store": True}


def wide():
    txt = wide_asm()
    with tempfile.TemporaryDirectory() as tmp:
        lab = os.path.join(tmp, "lab.s")
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                        "--cuda-device-only", os.path.join(REPO, "tools", "ubench", "tpi_lab.hip"), "-o", lab],
                       check=True, stderr=subprocess.DEVNULL)
        txt_m = open(lab).read()
    # the chain waves' phase loop: ONE sweep over the wave's row pair (55 distinct prefix rows of the pair's 84, three
    # ds_read_b64 each), the float64 finalisation and the stores of both rows, the barrier; an output row is half of it
    ph = chain_phase_loop(txt)
    mn = [x.split()[0] for x in ph]
    assert mn.count("ds_read_b64") == 3 * 55, "a row pair: 55 prefix rows of three reads"
    # the issue-priority ladder (WIDE_PRIO): 3, 2, 1, 0 over the sweep, back at 0 before the finalisation's stores
    ladder = ladder_report(ph)
    # a chain wave has no load in flight, only its output stores: a vmcnt wait in its phase loop can only wait for those
    # (round 10: the staging waves' last loads, open where the two paths meet, put four such waits there)
    vm_waits = [i for i, x in enumerate(ph) if x.startswith("s_waitcnt") and "vmcnt" in x]
    assert not vm_waits, f"the chain waves' phase loop waits for its output stores at instructions {vm_waits}"
    # nor may it grow: at most 812 VALU a pair (810 with the shared band sums alone; a scalar register that the staging
    # path's pressure pushes into a VGPR lane comes back here as a v_readlane, which is VALU and is reported beside the count)
    reloads = sum(x.startswith(("v_readlane", "v_writelane")) for x in mn)
    assert sum(x.startswith("v_") for x in mn) <= 812, f"the chain waves' phase loop grew ({reloads} reloads of spilled scalar registers in it)"
    # The phase boundary.  What ships is round 13's: slot, rows and lead fetches formed behind the barrier.  The lab switch
    # -DWIDE_BOUNDARY=1 (round 14: measured, not kept) is compiled and walked beside it so that it stays what was measured:
    # the lead fetches of the NEXT phase between the last output store and the barrier with no wait for them in front of it,
    # no multiplication and no reload of a spilled scalar on the hot path from the barrier to the sweep, and that path
    # shorter than the shipped one.
    lead_rows = probe_constant(txt, "wide_probe_lead_rows")
    boundary = boundary_report(txt, lead_rows)
    assert boundary["lead_reads_between_last_store_and_barrier"] == 0, "the shipped loop fetches in front of the barrier"
    lab_txt = wide_asm(["-DWIDE_BOUNDARY=1"])
    lab_mn = [x.split()[0] for x in chain_phase_loop(lab_txt)]
    lab = boundary_report(lab_txt, lead_rows)
    lab.update({"valu": sum(x.startswith("v_") for x in lab_mn), "ds_read_b64": lab_mn.count("ds_read_b64"),
                "salu": sum(x.startswith("s_") for x in lab_mn), "instructions": len(lab_mn)})
    assert lab["lead_reads_between_last_store_and_barrier"] == 3 * lead_rows, \
        f"WIDE_BOUNDARY=1: {lab['lead_reads_between_last_store_and_barrier']} reads between the last store and the barrier, not {3 * lead_rows}"
    assert not lab["lgkmcnt0_wait_between_lead_reads_and_barrier"], "WIDE_BOUNDARY=1: the lead fetches are waited for in front of the barrier"
    assert not lab["multiplies_and_readlanes_before_the_sweep"], \
        f"WIDE_BOUNDARY=1: behind the barrier, before the sweep: {lab['multiplies_and_readlanes_before_the_sweep']}"
    assert lab["hot_path_barrier_to_first_subtract"] < boundary["hot_path_barrier_to_first_subtract"], \
        "WIDE_BOUNDARY=1: the way from the barrier to the sweep is no shorter than the shipped one"
    boundary["lab_WIDE_BOUNDARY_1"] = lab
    row = ph
    o = mn
    # the staging waves' phase loop, and within it the lean path of an interior batch: its rows - from the first load to the
    # last, and from the first convert to the last ring write - are straight-line code with no select, no multiplication
    # and no 64-bit vector address (the one multiplication the scheduler may put among the rows is the batch's: its first
    # slot times the ring's row pitch of 0x600 bytes)
    st_all, st_lean = staging_loop(txt)
    lm = [x.split()[0] for x in st_lean]
    loads = [i for i, x in enumerate(lm) if x == "global_load_dwordx2"]
    first_cvt = lm.index("v_cvt_i32_f32_e32")
    last_write = max(i for i, x in enumerate(lm) if x.startswith("ds_write"))
    for name, (a, b) in {"loads": (loads[0], loads[-1]), "rows": (first_cvt, last_write)}.items():
        inside = lm[a:b + 1]
        assert not any(x.startswith(("s_cbranch", "s_branch")) for x in inside), f"lean path: a branch among the batch's {name}"
        muls = [x for x in st_lean[a:b + 1] if x.startswith(("s_mul", "v_mul", "v_mad"))]
        assert all(x.startswith("s_mul_i32") and x.endswith("0x600") for x in muls) and len(muls) <= (1 if name == "rows" else 0), \
            f"lean path: a multiplication per row among the batch's {name}: {muls}"
        assert "v_lshl_add_u64" not in inside, f"lean path: a 64-bit vector address among the batch's {name}"
    assert not any(x.startswith("v_cndmask") for x in lm[first_cvt:last_write + 1]), "lean path: a select among the batch's rows"
    # the classification (csrc/wide_classify.hpp) converts nothing back and compares nothing per sample: a row is two
    # v_fract_f32, one OR of three and one v_max3_f32 beside its converts and prefix adds; the batch's compares are on the
    # two accumulators (round 11 had 32 v_cvt_f32_i32 and 32 v_cmp_neq_f32 here, each compare with a scalar OR behind it)
    assert not any(x.startswith(("v_cvt_f32_i32", "v_cmp_neq_f32")) for x in lm), "lean path: a convert back or a compare per sample"
    assert sum(x.startswith("v_cmp") for x in lm) <= 6, "lean path: more compares than a batch's own (flags of two accumulators, lane 0's store)"
    assert sum(x.startswith("v_fract_f32") for x in lm) == 32 and sum(x.startswith("v_max3_f32") for x in lm) == 16, \
        "lean path: two v_fract_f32 and one v_max3_f32 a row"
    # The batch's branches, apart from the phase's own.  The staging of a batch comes first in a phase, then lane 0's store
    # of the flags (the one branch on the exec mask), then the next batch's loads, then the barrier; what follows the barrier
    # is the loop's.  In the source a batch makes three choices - lean or general staging, guard copies or none, interior
    # rows or not for the loads - and the compiler lays each two-sided choice out as the general block under one branch and
    # the lean block under a second one on a flag the first side sets: 2 + 1 branches for the staging, 2 for the loads.
    # (One branch per choice, two or three a batch, is what the source asks for; the second branch of a pair is the compiler's.)
    # the staging waves stand on top of the ladder while they stage: up before the batch's first convert, down again behind
    # its last ring write and before the wave waits at the barrier
    sp = [(i, int(x.split()[1])) for i, x in enumerate(st_lean) if x.startswith("s_setprio")]
    assert [l for _, l in sp] == [3, 0], f"lean path: the staging waves' priority goes {[l for _, l in sp]}, not 3 then 0"
    assert sp[0][0] < first_cvt and last_write < sp[1][0] < lm.index("s_barrier"), "lean path: raised before the first convert, lowered before the barrier"
    cond = [i for i, x in enumerate(lm) if x.startswith("s_cbranch")]
    flag_store = [i for i in cond if lm[i] == "s_cbranch_execz"]
    assert len(flag_store) == 1 and "s_barrier" in lm, "lean path: lane 0's flag store and the phase barrier mark the batch's parts"
    barrier = lm.index("s_barrier")
    assert last_write < flag_store[0] < loads[0] and loads[-1] < barrier, "lean path: staging, flag store, loads, barrier in this order"
    stage_branches = sum(1 for i in cond if i < flag_store[0])
    load_branches = sum(1 for i in cond if flag_store[0] < i < barrier)
    assert stage_branches <= 3, f"lean path: {stage_branches} branches for a batch's staging (lean or general twice, guard copies)"
    assert load_branches <= 2, f"lean path: {load_branches} branches for a batch's loads (interior rows or not, twice)"
    n_addr = address_adds(row)
    om = loop_ops(txt_m, KERNEL, lambda o: 42 <= sum(x == "ds_read_b128" for x in o) <= 46 and any("f64" in x for x in o))
    valu, kinds, ns = price(o)
    valu_m, kinds_m, ns_m = price(om)
    kinds["plain"] -= n_addr  # (plain adds: priced as before)
    kinds["ds_read_address"] = n_addr
    pair = {"valu": len(valu), "by_kind": dict(kinds), "ds_read_b64": o.count("ds_read_b64"), "s_nop": o.count("s_nop"),
            "salu": sum(1 for x in o if x.startswith("s_")), "global_store_dwordx2": o.count("global_store_dwordx2"),
            "vmcnt_waits": len(vm_waits), "sgpr_reloads": reloads, "instructions": len(o), "ns": round(ns, 1),
            "priority_ladder": ladder, "phase_boundary": boundary}
    # per output row: half the pair
    valu = valu[:len(valu) // 2]
    kinds = Counter({k: v / 2 for k, v in kinds.items()})
    ns /= 2
    # the strip's valid columns: WGeo<67>::TILE_W, read from the compiled unit's own constant
    cols, cols_m = probe_constant(txt, "wide_probe_tile_w"), TILE_W
    assert cols == 316, f"a strip's valid columns: {cols}, not 316"
    print(json.dumps({
        "kernel": "tpi_ring_wide_kernel<67>, one chain-wave row (316 columns: 52 lanes x 6 and a pair either side): half the row pair of the phase loop",
        "row_pair_instructions": pair,
        "staging_phase_loop": {"whole_loop": staging_report(st_all),
                               "lean_path": dict(staging_report(st_lean), batch_branches={"staging": stage_branches, "loads": load_branches},
                                                 priority={"levels": [l for _, l in sp], "raised_before_first_convert": True,
                                                           "lowered_before_barrier": True})},
        "row_loop_instructions": {"valu": pair["valu"] / 2, "by_kind": dict(kinds), "ds_read_b128": o.count("ds_read_b128") / 2,
                                  "ds_read_b64": o.count("ds_read_b64") / 2, "v_mov_b32_dpp": o.count("v_mov_b32_dpp") / 2,
                                  "s_nop": o.count("s_nop") / 2, "salu": sum(1 for x in o if x.startswith("s_")) / 2},
        "ns_per_wave_row": round(ns, 1),
        "valid_columns_per_wave_row": cols,
        "marching_kernel": {"kernel": "tpi_march_kernel<67, 60, 12, true, true, true>", "valu": len(valu_m), "by_kind": dict(kinds_m),
                            "ns_per_wave_row": round(ns_m, 1), "valid_columns_per_wave_row": cols_m},
        "valu_per_valid_column": {"wide": round(len(valu) / cols, 3), "marching": round(len(valu_m) / cols_m, 3)},
        "ns_per_valid_column": {"wide": round(ns / cols, 3), "marching": round(ns_m / cols_m, 3)},
        "valu_ns_per_valid_column_saved": round(1.0 - (ns / cols) / (ns_m / cols_m), 3),
        "issue_cost_ns_per_wave_instruction_and_simd": {"plain": NS_PLAIN, "half_rate": NS_HALF},
    }, indent=1))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "wide":
        return wide()
    std = len(sys.argv) > 1 and sys.argv[1] == "std"
    if std:
        del sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "lab.s")
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                        "--cuda-device-only", os.path.join(REPO, "tools", "ubench", "tpi_lab.hip"), "-o", asm],
                       check=True, stderr=subprocess.DEVNULL)
        txt = open(asm).read()
    start = txt.index((STD_KERNEL if std else KERNEL) + SUFFIX)
    lines = txt[start:txt.index("s_endpgm", start)].split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.search(r"s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))

    def ops(a, b):
        out = []
        for x in lines[a:b + 1]:
            x = x.strip()
            if x and not x.startswith((".", ";", "//")) and not x.endswith(":"):
                out.append(x.split()[0])
        return out

    # the row loop: the innermost loop with the chain's 42 prefix-row reads (+ 2 for the pixel's own value) that also
    # converts to float64 (the whole-metre copy of the loop; the sums-only copy for fractional tiles does not)
    best = None
    for a, b in loops:
        o = ops(a, b)
        reads = sum(1 for x in o if x == "ds_read_b128")
        if std:
            # the phase loop: the smallest loop that holds both chains' prefix-row reads and the phase's barriers
            if reads >= 84 and sum(1 for x in o if x == "s_barrier") >= 2 and (best is None or b - a < best[1] - best[0]):
                best = (a, b)
        elif 42 <= reads <= 46 and any("f64" in x for x in o):
            if best is None or b - a < best[1] - best[0]:
                best = (a, b)
    o = ops(*best)
    valu = [x for x in o if x.startswith("v_")]
    mix = Counter("half" if half_rate(x) else "plain" for x in valu)
    kinds = Counter()
    for x in valu:
        kinds["dpp" if "_dpp" in x else "add3" if "add3" in x else "f64_or_convert" if ("f64" in x or x.startswith("v_cvt")) else
              "other_half_rate" if half_rate(x) else "plain"] += 1
    ns_row = mix["plain"] * NS_PLAIN + mix["half"] * NS_HALF
    tiles = ((NX + TILE_W - 1) // TILE_W) * (NY // TH + (1 if NY % TH else 0))
    wave_rows = tiles * TH
    total_valu = None
    if len(sys.argv) > 1:
        total_valu = float(sys.argv[1])
    else:
        try:
            block = open(os.path.join(REPO, "profiles", "r06_std67_pmc_summary.txt" if std else "r06_tpi67_pmc_summary.txt")).read() \
                .split("std_ring_kernel<67, false" if std else "tpi_march_kernel<67")[1]
            total_valu = float(re.search(r"SQ_INSTS_VALU\s+n=\s*\d+\s+mean=([0-9.e+]+)", block).group(1))
        except (OSError, IndexError, AttributeError):
            pass
    row_instr = len(valu) * wave_rows
    ms_rows = ns_row * wave_rows / 1024 / 1e6
    result = {
        "kernel": "std_ring_kernel<67, false, kStdMain>, phase loop (one output row per wave and phase)" if std else
                  "tpi_march_kernel<67, 60, 12, true, true, true>, row loop (whole-metre tiles)",
        "row_loop_instructions": {"valu": len(valu), "by_kind": dict(kinds), "ds_read_b128": sum(1 for x in o if x == "ds_read_b128"),
                                  "salu": sum(1 for x in o if x.startswith("s_"))},
        "issue_cost_ns_per_wave_instruction_and_simd": {"plain": NS_PLAIN, "half_rate": NS_HALF,
                                                        "source": "profiles/r02_valu_mix_rate.txt, profiles/r03_valu_mix2_rate.txt (16 waves per CU, wall clock)"},
        "ns_per_wave_row": round(ns_row, 1),
        "wave_rows_per_launch": wave_rows,
        "row_loop_valu_bound_ms": round(ms_rows, 3),
    }
    if total_valu and std:
        # the phase loop holds branches only some waves take (waves 0-3 stage, convert and write the ring rows for all
        # twelve), so its static count overstates a wave's work: the launch's counter, priced at the loop's mix, is the bound
        avg = ns_row / len(valu)
        result.update({"SQ_INSTS_VALU_per_launch": total_valu,
                       "static_count_x_wave_rows": row_instr,
                       "note": "the static count includes the staging share only waves 0-3 execute; the bound prices the "
                               "launch's SQ_INSTS_VALU at the phase loop's mix of issue classes",
                       "ns_per_valu_instruction_at_this_mix": round(avg, 3),
                       "valu_bound_ms": round(total_valu * avg / 1024 / 1e6, 3)})
    elif total_valu:
        rest = max(0.0, total_valu - row_instr)
        avg = ns_row / len(valu)
        ms_rest = rest * avg / 1024 / 1e6
        result.update({"SQ_INSTS_VALU_per_launch": total_valu, "valu_outside_the_row_loop": rest,
                       "outside_valu_bound_ms": round(ms_rest, 3), "valu_bound_ms": round(ms_rows + ms_rest, 3)})
    else:
        result["valu_bound_ms"] = round(ms_rows, 3)
    import bench
    result["kernel_sources_sha256"] = bench.kernel_sources_sha256()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

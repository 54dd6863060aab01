"""usage: python tools/isa_body_regions.py file.s [kernel-substring [body-file]]
Static counts of the large-form kernels' assembly (hipcc -S --cuda-device-only -gline-tables-only with the Makefile's flags).
Every instruction is attributed to the last .loc of wpt_pathtrace_body.inc.h in front of it (an inlined function's
instructions so count for the body line that called it), and the body lines are cut into regions at the marker comments of
the source, so that the regions stay what they are when lines move:
  prologue    up to the pool's lambda: the copies to LDS, the pixel's start (and whatever follows a line of it unmarked)
  pool/head   the pool's lambda and the outer loop's head: what the compiler sets up in front of the loop, run once
  look        from "the wave's scheduler" to the walk's pick           (the scheduler's look, once per iteration)
  walk        the traversal block
  shade, nee  the two hit blocks of the long round (their inlined functions mostly follow other lines)
  new         from "last: in a fused round" to the rays' start         (the new-sample block)
  begin       the rays' start
Per kernel and region: vector instructions, lane-spill instructions among them (v_readlane_b32 / v_writelane_b32), v_mul_f32
among them (a cue for the quatRotate expansions: one is 18 multiplications), scalar, ds and memory instructions.  The head
line of a kernel has its vgpr_count, sgpr_spill_count, vgpr_spill_count and scratch bytes from the metadata.  The assembly
must be that of the tree the tool runs in: the regions are cut by this tree's line numbers."""
import os
import re
import sys

BODY = "wpt_pathtrace_body.inc.h"
MARKS = [("prologue", None), ("pool/head", "idle lanes take the next pixels of the launch"), ("look", "---- the wave's scheduler ----"), ("walk", "if (pick == S_NODE) {"),
         ("shade", "if (pick != S_NODE && (fused ? cShade > 0"), ("nee", "if (pick != S_NODE && (fused ? cNee > 0"),
         ("new", "/* last: in a fused round it also serves"), ("begin", "sec<COUNT>(lc, SEC_BEGIN_RAY"), ("end", "if (COUNT && args.counters && inBlock)")]


def region_starts(body_path):
    starts = []
    lines = open(body_path).read().split("\n")
    for name, mark in MARKS:
        if mark is None:
            starts.append((1, name))
            continue
        at = [i + 1 for i, l in enumerate(lines) if mark in l]
        assert len(at) == 1, (mark, at)
        starts.append((at[0], name))
    return starts


def region_of(starts, line):
    name = starts[0][1]
    for at, n in starts:
        if line >= at:
            name = n
    return name


def main():
    s_path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "wpt_pathtrace_large"
    # (a third argument: the body file the assembly was compiled from, for the assembly of another commit)
    body = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "wurblpt_amd", "csrc", BODY)
    starts = region_starts(body)
    body_ids = set()
    kernel, region, counts, order = None, "prologue", {}, []
    meta = {}
    name = None
    for line in open(s_path):
        t = line.strip()
        m = re.match(r'\.file\s+(\d+)\s+.*"([^"]*)"', t)
        if m and m.group(2).endswith(BODY):
            body_ids.add(int(m.group(1)))
            continue
        m = re.match(r"^(_Z\w*):", t)
        if m:
            kernel = m.group(1) if want in m.group(1) else None
            if kernel:
                counts[kernel] = {}
                order.append(kernel)
                region = "prologue"
            continue
        if t.startswith(".Lfunc_end"):
            kernel = None
            continue
        m = re.match(r"\.name:\s+(\S+)", t)
        if m:
            name = m.group(1)
        m = re.match(r"\.(sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size|sgpr_count):\s+(\d+)", t)
        if m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
        if not kernel:
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            if int(m.group(1)) in body_ids:
                region = region_of(starts, int(m.group(2)))
            continue
        m = re.match(r"^(v_|s_|ds_|global_|buffer_|scratch_|flat_)(\w*)", t)
        if not m:
            continue
        c = counts[kernel].setdefault(region, dict(valu=0, lane=0, salu=0, lds=0, mem=0, mul=0))
        op = m.group(1) + m.group(2)
        if m.group(1) == "v_":
            c["valu"] += 1
            if op in ("v_readlane_b32", "v_writelane_b32"):
                c["lane"] += 1
            if op.startswith("v_mul_f32"):
                c["mul"] += 1
        elif m.group(1) == "s_":
            c["salu"] += 1
        elif m.group(1) == "ds_":
            c["lds"] += 1
        else:
            c["mem"] += 1
    for k in order:
        mk = meta.get(k, {})
        print("%s  vgpr %s sgpr_spill %s vgpr_spill %s scratch %s" % (k, mk.get("vgpr_count"), mk.get("sgpr_spill_count"), mk.get("vgpr_spill_count"),
              mk.get("private_segment_fixed_size")))
        for _, r in starts:
            c = counts[k].get(r)
            if c:
                print("    %-9s valu %4d  lane-spill %3d  v_mul_f32 %3d  salu %4d  ds %3d  mem %3d" % (r, c["valu"], c["lane"], c["mul"], c["salu"], c["lds"], c["mem"]))


if __name__ == "__main__":
    main()

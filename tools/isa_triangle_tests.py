"""Static instruction counts of the triangle tests of an LDS kernel, from assembly with line tables:
  hipcc --offload-arch=gfx950 <HIPFLAGS of wurblpt_amd/csrc/Makefile for the unit> -mllvm -disable-machine-licm -gline-tables-only -S --cuda-device-only
        wurblpt_amd/csrc/wpt_k_basic_lds[_rot].hip -o X.s
usage: python tools/isa_triangle_tests.py X.s LABEL=REGEX ...   (REGEX is matched against an instruction's .loc line with its inlining chain,
e.g. 'leaf=wpt_pathtrace\\.inc\\.h:586:' for everything inlined into the call on that line)"""
import re
import sys


def count(path, sections):
    loc, out = "", {k: {} for k in sections}
    for line in open(path):
        s = line.strip()
        if s.startswith(".loc"):
            loc = s
            continue
        m = re.match(r"(v_\w+|s_\w+|ds_\w+)", s)
        if not m:
            continue
        op = m.group(1)
        for sec, pat in sections.items():
            if re.search(pat, loc):
                kind = ("v_cndmask_b32" if op.startswith("v_cndmask") else "v_cmp" if op.startswith("v_cmp") else "v_pk" if op.startswith("v_pk")
                        else "v_mov" if op.startswith("v_mov") else "other VALU" if op.startswith("v_") else op if op.startswith("ds_") else "SALU")
                out[sec][kind] = out[sec].get(kind, 0) + 1
                break
    return out


if __name__ == "__main__":
    path = sys.argv[1]
    sections = dict(a.split("=", 1) for a in sys.argv[2:])
    for key in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size"):
        for line in open(path):
            if line.strip().startswith(key + ":"):
                print("  " + line.strip())
                break
    for sec, d in count(path, sections).items():
        valu = sum(n for k, n in d.items() if k.startswith("v_") or k == "other VALU")
        print("  %s: VALU %d (%s)" % (sec, valu, ", ".join("%s %d" % kv for kv in sorted(d.items()))))

"""Generates tests/golden/obj/fuzz_ref.json: what the reference's own OBJ / MTL parser (tiny_obj_loader.h, through
oracle/_ref/ref_probe --obj, which build() compiles where the reference tree exists) reads from the 60 random OBJ / MTL
pairs of tests/test_import.py (_random_obj, seed 31), one case per line.  Run from the repository root after build()."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests.test_import import OBJ_FUZZ_CASES, OBJ_FUZZ_SEED, _random_obj  # noqa: E402

if __name__ == "__main__":
    probe = os.path.join(ROOT, "oracle", "_ref", "ref_probe")
    rng = np.random.default_rng(OBJ_FUZZ_SEED)
    cases = []
    with tempfile.TemporaryDirectory() as d:
        for case in range(OBJ_FUZZ_CASES):
            obj = _random_obj(rng, d, "case%d" % case)
            out = os.path.join(d, "ref.json")
            subprocess.run([probe, "--obj", obj, out], check=True, timeout=60, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            ref = json.load(open(out))
            del ref["generator"]
            cases.append(json.dumps(ref, sort_keys=True, separators=(",", ":")))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "obj", "fuzz_ref.json")
    with open(path, "w") as f:
        f.write('{"generator": "oracle/ref_probe.cpp --obj", "seed": %d, "cases": [\n%s\n]}\n' % (OBJ_FUZZ_SEED, ",\n".join(cases)))

#!/usr/bin/env python3
"""Record what the reference computes for tests/test_reference_differential.py: runs each of that module's
reference-side scripts on a reference tree, over the default seed range of its test, and writes the JSON results to
tests/golden/reference_differential.json.gz.

TEST INFRASTRUCTURE.  Run where a reference tree exists:
    ART_REFERENCE=<reference tree> python tests/golden/generate_reference_differential.py
The test then reads the recorded results and needs no reference tree; each record carries a hash of the script and
generator text it came from, and the test refuses a record whose text has changed since.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))

import test_reference_differential as T  # noqa: E402

# key -> (script, text on its stdin, seed range): the defaults of the tests' ART_FUZZ_* variables
CASES = {
    "placements": (T.REF_SCRIPT, T.GENERATOR, (0, 60)),
    "focus": (T.FOCUS_SCRIPT, T.GENERATOR, (0, 24)),
    "ops": (T.OPS_SCRIPT, T.GENERATOR + T.OPS_GEN, (0, 30)),
    "methods": (T.METHODS_SCRIPT, T.METHODS_GEN, (0, 48)),
    "detector": (T.DET_SCRIPT, T.GENERATOR + T.DET_GEN, (0, 40)),
    "errors": (T.ERR_SCRIPT, T.ERR_PRELUDE + "#CASES#" + json.dumps(T.ERR_CASES), (None, None)),
    "geometry": (T.GEO_SCRIPT, T.GEO_GEN, (0, 60)),
    "main": (T.MAIN_SCRIPT, T.GENERATOR + T.MAIN_GEN, (0, 24)),
}


def main():
    ref_tree = os.environ.get("ART_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref_tree or not os.path.isdir(ref_tree):
        sys.exit("usage: ART_REFERENCE=<reference tree> python tests/golden/generate_reference_differential.py")
    out = {}
    for key, (script, stdin, (lo, hi)) in CASES.items():
        print(f"[golden] {key} seeds [{lo}, {hi})", flush=True)
        out[key] = {"range": [lo, hi], "script_sha256": T.script_key(script, stdin),
                    "result": T.run_reference(ref_tree, script, stdin, lo, hi)}
    path = os.path.join(HERE, "reference_differential.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print(f"[golden] wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

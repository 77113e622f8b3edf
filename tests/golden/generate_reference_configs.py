#!/usr/bin/env python3
"""Record the option dictionaries of the reference's shipped CONFIG_*.py scripts for tests/test_reference_configs.py:
each script is executed on the reference tree and its SourceProperties / DetectorOptions / AnalysisOptions are written,
key for key, to tests/golden/reference_configs.json.  (Two scripts pass a 7th positional `render` argument that the
reference's OEPlacement rejects; it is dropped here so that their dictionaries can be read.)

TEST INFRASTRUCTURE.  Run where a reference tree exists:
    ART_REFERENCE=<reference tree> python tests/golden/generate_reference_configs.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
CONFIGS = ["CONFIG_singleparabola.py", "CONFIG_2toroidals_f-x-f.py", "CONFIG_2toroidals_twisted.py",
           "CONFIG_toroidal2f-2f.py", "CONFIG_toroidal2f-2f_byhand.py", "CONFIG_CollimatingTelescope.py",
           "CONFIG_deformed.py"]


def main():
    ref_tree = os.environ.get("ART_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref_tree or not os.path.isdir(ref_tree):
        sys.exit("usage: ART_REFERENCE=<reference tree> python tests/golden/generate_reference_configs.py")
    sys.path[:0] = [ref_tree, os.path.join(HERE, "_standin")]
    import matplotlib
    matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleProcessing as mp
    assert mp.__file__.startswith(os.path.abspath(ref_tree))
    placement = mp.OEPlacement
    mp.OEPlacement = lambda *a, **k: placement(*a[:6], **k)
    np.random.seed(1)
    out = {}
    for name in CONFIGS:
        spec = importlib.util.spec_from_file_location(name[:-3], os.path.join(ref_tree, "examples", name))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out[name] = {k: getattr(mod, k) for k in ("SourceProperties", "DetectorOptions", "AnalysisOptions")}
    path = os.path.join(HERE, "reference_configs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, default=float)
        f.write("\n")
    print(f"[golden] wrote {path}")


if __name__ == "__main__":
    main()

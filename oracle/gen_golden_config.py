"""Generate tests/golden/configs.json from the reference's project configs (build container only).

    python -m oracle.gen_golden_config

For every projects/{Supervised,MonoDepth2}/configs/*.yaml: the mapping yaml.safe_load reads from the file (anchors resolved, the
``_BASE_`` entry kept), keyed "<project>/<file name>".  tests/test_config.py writes these back out as YAML files and merges them.
"""
import glob
import json
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "configs.json")


def main():
    res = {}
    for project in ("Supervised", "MonoDepth2"):
        for path in sorted(glob.glob(os.path.join(ref_harness.REF_ROOT, "projects", project, "configs", "*.yaml"))):
            with open(path) as f:
                res[f"{project}/{os.path.basename(path)}"] = yaml.safe_load(f) or {}
    assert res, f"no project configs under {ref_harness.REF_ROOT}"
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(res)} configs to {OUT}")


if __name__ == "__main__":
    main()

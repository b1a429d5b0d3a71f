"""CPU-only: the committed profile of tools/linear_ce_bench.py (profiles/r06_linear_ce_bench.json, which DESIGN.md section 4.4.2 quotes) was
measured on the ce_fused.hip of this tree, its --check held on every shape, and the built-in default chunk_rows is what the rule of
DESIGN.md picks from the recorded sweep. A change to ce_fused.hip fails here until the tool is run again."""
import json
from pathlib import Path

import bench
import kfunca_amd as kfunca

ROOT = Path(__file__).resolve().parent.parent


def test_the_committed_bench_profile_was_measured_on_this_source():
    obj = json.loads((ROOT / "profiles" / "r06_linear_ce_bench.json").read_text())
    assert bench.stamp_is_current(obj, ("ce_fused.hip",)), "profiles/r06_linear_ce_bench.json is stale: re-run tools/linear_ce_bench.py --check"
    assert len(obj["cases"]) == 4 and all(c["check"]["ok"] for c in obj["cases"])
    assert obj["default_rule"]["picks"] == kfunca._linear_ce_chunk_rows(0)

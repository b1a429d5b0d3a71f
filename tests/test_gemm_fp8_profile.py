"""CPU-only: the committed profile of tools/gemm_fp8_bench.py (profiles/r06_gemm_fp8_bench.json, which DESIGN.md section 4.12 quotes) was
measured on the fp8.hip and gemm_fp8.hip of this tree, its --check held on every shape, and the accumulation term of tests/fp8_ref.py is
at least twice the worst block-sum figure it recorded. A change to either source fails here until the tool is run again."""
import json
from pathlib import Path

import bench
from tests import fp8_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_the_committed_bench_profile_was_measured_on_this_source():
    obj = json.loads((ROOT / "profiles" / "r06_gemm_fp8_bench.json").read_text())
    assert bench.stamp_is_current(obj, ("fp8.hip", "gemm_fp8.hip")), "profiles/r06_gemm_fp8_bench.json is stale: re-run tools/gemm_fp8_bench.py --check"
    assert len(obj["gemm"]) == 5 and all(c["check"]["ok"] for c in obj["gemm"])
    assert len(obj["quantize"]) == 2 and len(obj["linear"]) == 5
    worst = max(b["worst_err_over_mag"] for b in obj["block_sum"])
    assert len(obj["block_sum"]) == 8 and 2 * worst <= R.ACC_TERM == obj["acc_term"], (worst, R.ACC_TERM)

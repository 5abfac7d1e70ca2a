"""profiles/illum_parity.json from the margins file that a GPU run of the suite leaves behind (tests/parity.py, dump_margins): per test of
tests/test_gpu_illum.py, the case whose device - rule difference comes closest to its bar (parity.BIN_RTOL for the map, 1e-9 for the line,
max(16 x noise, floor) for the response).

  python scripts/illum_parity_worst.py <margins.json> [<out.json>]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = ("test_map_of_traced_sources_equals_the_rule", "test_line_with_a_table_against_the_rule", "test_response_with_a_table_against_the_rule",
         "test_every_instance_of_the_table_response", "test_axisymmetric_table_is_the_flat_twin", "test_phase_is_a_roll_of_the_table",
         "test_api_line_profile_and_disc_response_with_a_table")


def main():
    src = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "illum_parity.json")
    rows = [r for r in json.load(open(src))["rows"] if r["test"] in TESTS]
    keep = ("test", "case", "n_traced", "worst_ok", "allowed_bad_frac", "noise", "floor")
    worst = [max((r for r in rows if r["test"] == name), key=lambda r: r["worst_ok"] / r["allowed_bad_frac"]) for name in TESTS if any(r["test"] == name for r in rows)]
    with open(out, "w") as f:
        json.dump({"what": "per test, the case whose device - rule difference (worst_ok) comes closest to its bar (allowed_bad_frac) (tests/test_gpu_illum.py)",
                   "cases": len(rows), "rows": [{k: r[k] for k in keep if k in r} for r in worst]}, f, indent=1)
    print(f"{len(rows)} comparisons, {len(worst)} tests -> {out}")


if __name__ == "__main__":
    main()

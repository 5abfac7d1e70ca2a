"""profiles/reverb_response_parity.json from the margins file that a GPU run of the suite leaves behind (tests/parity.py, dump_margins): per test of
tests/test_gpu_reverb_response.py, the case whose device - rule difference comes closest to its bar max(16 x noise, floor).

  python scripts/response_parity_worst.py <margins.json> [<out.json>]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    src = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reverb_response_parity.json")
    rows = [r for r in json.load(open(src))["rows"] if "cells" in r and "outside" in r]          # the extras only the response comparisons record
    tests = sorted({r["test"] for r in rows})
    worst = [max((r for r in rows if r["test"] == name), key=lambda r: r["worst_ok"] / r["allowed_bad_frac"]) for name in tests]
    with open(out, "w") as f:
        json.dump({"what": "per test, the case whose device - rule difference comes closest to its bar max(16 x noise, floor) (tests/test_gpu_reverb_response.py)",
                   "cases": len(rows), "largest_device_minus_rule": max(r["worst_ok"] for r in rows), "rows": worst}, f, indent=1)
    print(f"{len(rows)} comparisons, {len(worst)} tests -> {out}")


if __name__ == "__main__":
    main()

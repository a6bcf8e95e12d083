"""Record tests/golden/plan_shapes.json: what ``engine.Plan(...).info`` reports for every case of
tests/plan_cases.py on this build and this GPU, with the two facts of the device and the reads
that the planner depends on (compute units; reads of one width).

    python tools/record_plan_shapes.py [OUT.json]

Run it on the commit whose plans are the reference (the parent of a planner refactor).  Needs the
GPU: a tool, not a test.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import plan_cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_shapes.json")
    rec = {"n_cus": torch.cuda.get_device_properties(0).multi_processor_count, "cases": []}
    for vid, case, uniform in plan_cases.variants():
        rs, plan = plan_cases.build_plan(case, uniform)
        info = {k: int(v) for k, v in plan.info.items() if k != "reserved"}
        rec["cases"].append({"id": vid, "uniform": uniform, "info": info})
        plan.close()
        rs.close()
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d plans -> %s" % (len(rec["cases"]), out))


if __name__ == "__main__":
    main()

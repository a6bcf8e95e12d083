"""The library's plans against tests/golden/plan_shapes.json: ``engine.Plan(...).info`` of every
case of tests/plan_cases.py, as recorded by tools/record_plan_shapes.py.  With
tests/test_plan_shape.py, which holds the stand-alone planner to the same fixture, the driver,
the library and the recording agree.  Plan creation alone: no kernel of a plan runs."""
import json
import os

import pytest
import torch

from tests import plan_cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_shapes.json")) as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["id"]: c for c in GOLDEN["cases"]}
VARIANTS = plan_cases.variants()


def test_fixture_was_recorded_on_this_device(gpu):
    """The planner sizes grids and rounds by the compute units: the fixture holds for its device."""
    assert torch.cuda.get_device_properties(0).multi_processor_count == GOLDEN["n_cus"]


@pytest.mark.parametrize("vid,case,uniform", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_plan_info_is_the_recorded_one(gpu, vid, case, uniform):
    rs, plan = plan_cases.build_plan(case, uniform)
    try:
        info = {k: int(v) for k, v in plan.info.items() if k != "reserved"}
    finally:
        plan.close()
        rs.close()
    assert info == EXPECTED[vid]["info"]

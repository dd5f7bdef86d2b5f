"""Every apply of the grid of calls in tests/golden/make_apply_choices.py launches the kernel the golden recorded.

tests/golden/apply_choices.json holds (last_kernel, last_launch) of every call -- matrices on either side of each threshold of the
choice, the field and batch counts, the per-handle options one at a time, set_kernel requests, a first and a second apply and one
after prepare -- as recorded at the commit named inside it, before the choice moved into apply_plan.h.  The results of the applies
are not compared here (tests/test_gpu_apply_kernels.py, tests/test_gpu_parity.py)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_apply_choices as mac  # noqa: E402

pytestmark = pytest.mark.gpu

with open(mac.OUTPUT) as _f:
    GOLDEN = json.load(_f)


def test_golden_names_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(c["id"] for c in mac.CASES)
    assert len(GOLDEN["commit"]) == 40


@pytest.mark.parametrize("case", mac.CASES, ids=[c["id"] for c in mac.CASES])
def test_apply_choice(case):
    want = iter(GOLDEN["cases"][case["id"]])
    got = mac.record(case)
    assert 3 * len(got) == len(GOLDEN["cases"][case["id"]])
    for nvar, nbatch, seen in got:
        for state, s in zip(("first apply", "second apply", "after prepare"), seen):
            assert "%s|%s" % s == GOLDEN["names"][next(want)], (case["id"], nvar, nbatch, state)

"""The GEMM route matrix of tests/test_gpu_gemm_routes.py, checked on the CPU: the float64 oracle is the plain product, the recorded
bounds are 4 x what the float32 running sum loses at every case (neither stale nor loose), and the comparison is sharp -- every
mutation of helpers.GEMM_BUGS that applies to a case lands at least 10 x above that case's bound.  No GPU."""
import pytest
import torch

import helpers
from helpers import GEMM_BOUND, GEMM_BUGS, GEMM_CASES, GEMM_FLOORS, GEMM_VARIANTS

IDS = [c["id"] for c in GEMM_CASES]


def test_the_table_covers_every_route_and_every_mutation():
    assert len(set(IDS)) == len(IDS) and set(GEMM_FLOORS) == set(IDS)
    assert {c["route"][0] for c in GEMM_CASES} == set(helpers.GEMM_ROUTES_COVERED)
    assert {b for c in GEMM_CASES for b in c["bugs"]} == set(GEMM_BUGS)
    for c in GEMM_CASES:
        assert c["fixed"][0] not in helpers.GEMM_SPLITTING and c["fixed"][1] == 1, c["id"]
        assert (c["no_mid"] is not None) == (c["route"][0] == "mid-split"), c["id"]
        assert (c["no_streamk"] is not None) == (c["route"][0].startswith("streamk") or c["route"][0] == "splitk"), c["id"]
    print("\ncase: mutations that apply")
    for c in GEMM_CASES:
        print(f"  {c['id']:38s} {' '.join(c['bugs'])}")


@pytest.mark.parametrize("case", GEMM_CASES, ids=IDS)
def test_float32_floors(case):
    """the recorded bound is between 2 x and 8 x the floor recomputed here (the larger of the two alignment variants')"""
    floors = [helpers.gemm_floor(case, v) for v in GEMM_VARIANTS]
    bound = GEMM_BOUND[case["id"]]
    print(f"\nMEASURED {case['id']}: float32 floor {floors[0]:.3g} (aligned) {floors[1]:.3g} (odd), bound {bound:.3g}")
    assert bound == 4.0 * GEMM_FLOORS[case["id"]]
    assert 2.0 * max(floors) <= bound <= 8.0 * max(floors)


@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("case", GEMM_CASES, ids=IDS)
def test_every_mutation_is_at_least_ten_bounds_away(case, variant):
    rows = helpers.gemm_sample_rows(case) if case["sample"] else None
    ref = helpers.gemm_oracle(case, torch.float64, variant, rows=rows)
    den = helpers.gemm_denominator(case, variant, rows)
    bound = GEMM_BOUND[case["id"]]
    for bug in case["bugs"]:
        mut = helpers.gemm_oracle(case, torch.float64, variant, bug=bug, rows=rows)
        touched = mut != ref
        assert bool(touched.any()), (case["id"], bug)
        err, where = helpers.gemm_error(mut, ref, den)
        print(f"{case['id']} {bug}: {int(touched.sum())} elements, worst {err:.3g} = {err / bound:.3g} bounds at {where}")
        assert err >= 10.0 * bound, (case["id"], variant, bug, err, bound)
        # ... and the float32 evaluation of the mutant is as far off: float32 rounding cannot mend it
        mut32 = helpers.gemm_oracle(case, torch.float32, variant, bug=bug, rows=rows)
        assert helpers.gemm_error(mut32, ref, den)[0] >= 10.0 * bound, (case["id"], variant, bug)


@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("case", [c for c in GEMM_CASES if c["alpha"] == 1.0 and c["beta"] == 0.0 and not c["bias"]
                                  and c["nbatch"] == 1 and c["lda"] is None], ids=helpers.gemm_case_id)
def test_float64_oracle_is_the_plain_product(case, variant):
    """on the plain cases the oracle IS A.double() @ B.double(), with A and B gathered here element by element from the buffers the
    device gets (an index table, not the oracle's strided view)"""
    d = helpers.gemm_case_data(case, variant)
    M, N, K = case["M"], case["N"], case["K"]
    rows = helpers.gemm_sample_rows(case) if case["sample"] else torch.arange(M)
    (sam, sak), (sbk, sbn) = d["sa"], d["sb"]
    A = d["A"][d["off"] + rows[:, None] * sam + torch.arange(K)[None, :] * sak]
    B = d["B"][d["off"] + torch.arange(K)[:, None] * sbk + torch.arange(N)[None, :] * sbn]
    assert torch.equal(helpers.gemm_oracle(case, torch.float64, variant, rows=rows)[0], A.double() @ B.double())

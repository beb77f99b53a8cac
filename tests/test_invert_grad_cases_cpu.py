"""The sweep of test_invert_grad_gpu.py reaches every dispatch class invert_grad_cases.py names, in both forms, and its
many-rows cases make the kernel's row loop turn at least three times with a partial last trip."""
import grad_cases as G
import invert_grad_cases as C


def _plans(cases, polar):
    return {name: C.module_plan(G.magnitude_module(kw), polar) for name, kw, _ in cases}


def test_real_sweep_reaches_every_class():
    plans = _plans(C.MAG_CASES, False)
    assert {p[0] for p in plans.values()} == C.REAL_CLASSES
    assert plans["n1024_off"][0] == plans["n8192_off"][0] == "pointwise"
    assert plans["n2048_nonyq"][0] == "lds" and plans["n8192"][0] == "lds_big" and plans["n16384"][0] == "global_w4"
    assert all(lds <= C.LDS_BUDGET for _, _, lds in plans.values())


def test_polar_sweep_reaches_every_class():
    assert len(C.POLAR_CASES) >= 8 and all(C.polar_eligible(kw) for _, kw, _ in C.POLAR_CASES)
    plans = _plans(C.POLAR_CASES, True)
    assert {p[0] for p in plans.values()} == C.POLAR_CLASSES
    assert plans["n4096"][0] == "global_w4" and plans["n8192"][:2] == ("global_w3", 3)
    assert plans["n16384"][:2] == ("global_w1", 1)
    assert all(lds <= C.LDS_BUDGET for _, _, lds in plans.values())


def test_fewer_waves_cannot_happen_in_the_real_form():
    """A wave's slice is g alone: at the largest N the library takes, four of them fit the budget."""
    assert 4 * C.per_wave_bytes(8193, 8193, False) <= C.LDS_BUDGET
    assert C.launch_plan(8193, 8193, 10 ** 6)[0] == "global_w4"


def test_rows_that_leave_waves_idle_are_in_the_sweep():
    rows = {name: r for name, _, r in C.MAG_CASES}
    assert rows["rows1"] == (1, 1) and rows["rows3"] == (1, 3) and rows["rows5"] == (1, 5)
    assert all(r in ((2, 5), (1, 3)) for name, r in rows.items() if not name.startswith("rows"))


def test_many_rows_make_three_trips_and_a_partial_last_one():
    for form, (kw, rows) in C.MANY_ROWS.items():
        cls, wpb, lds = C.module_plan(G.magnitude_module(kw), form == "polar")
        assert cls == "lds" and wpb == 4
        trips, last = C.row_loop_trips(rows[0] * rows[1], wpb, lds)
        assert trips >= 3 and 0 < last < C.grid_blocks(rows[0] * rows[1], wpb, lds), (form, trips, last)

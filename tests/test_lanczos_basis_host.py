"""The host-side pieces of the kept Lanczos basis (``eigensolvers_amd/lanczos_filter.py``): the byte budget, the splitting
of wide coefficient tables into calls, and the ``ValueError`` paths that need no device.

Every case fails without the feature: the names do not exist."""
import importlib

import numpy as np
import pytest

lf = importlib.import_module("eigensolvers_amd.lanczos_filter")       # the package exports the function of the same name

GB = 1 << 30


def test_budget_is_nine_tenths_of_free_plus_reusable_bytes():
    assert lf.BASIS_SAFETY == 0.9
    assert lf.basis_budget(100 * GB, 0) == int(0.9 * 100 * GB)
    assert lf.basis_budget(100 * GB, 20 * GB) == int(0.9 * 120 * GB)
    assert lf.basis_budget(0, 20 * GB) == int(0.9 * 20 * GB)
    assert lf.basis_budget(1000, 0) == 900 and isinstance(lf.basis_budget(1000, 0), int)


def test_budget_with_zero_free_memory_is_zero():
    assert lf.basis_budget(0, 0) == 0
    assert lf.basis_budget(-5, 0) == 0            # a driver that reports nonsense gives no room, never a negative budget


def test_budget_override_replaces_the_device_figures_and_counts_what_the_run_holds():
    assert lf.basis_budget(100 * GB, 20 * GB, override=12345) == 12345
    assert lf.basis_budget(0, 0, override=12345) == 12345
    assert lf.basis_budget(100 * GB, 0, override=1000, held=400) == 600
    assert lf.basis_budget(100 * GB, 0, override=1000, held=1000) == 0
    assert lf.basis_budget(100 * GB, 0, override=1000, held=5000) == 0
    assert lf.basis_budget(100 * GB, 0, override=0) == 0
    with pytest.raises(ValueError):
        lf.basis_budget(100 * GB, 0, override=-1)


def test_budget_is_a_pure_function():
    args = (123456789, 987654, None, 0)
    assert lf.basis_budget(*args) == lf.basis_budget(*args) == int(0.9 * (123456789 + 987654))


@pytest.mark.parametrize("nc,calls", [(1, [(0, 1)]), (2, [(0, 2)]), (3, [(0, 2), (2, 1)]), (4, [(0, 4)]), (8, [(0, 8)]),
                                      (11, [(0, 8), (8, 2), (10, 1)]), (16, [(0, 8), (8, 8)]),
                                      (7, [(0, 4), (4, 2), (6, 1)])])
def test_wide_tables_are_split_into_calls(nc, calls):
    got = lf.split_combinations(nc)
    assert got == calls
    assert all(w in (1, 2, 4, 8) for _, w in got)
    covered = [c for lo, w in got for c in range(lo, lo + w)]
    assert covered == list(range(nc))             # every column of the table once, in order


def test_no_combination_is_refused():
    with pytest.raises(ValueError):
        lf.split_combinations(0)


def test_basis_mode_values():
    assert lf.BASIS_MODES == ("recompute", "keep")
    for ok in lf.BASIS_MODES:
        assert lf._checked_basis_mode(ok, "basis") == ok
    for bad in ("kept", "Keep", None, True, ""):
        with pytest.raises(ValueError, match="basis"):
            lf._checked_basis_mode(bad, "basis")


def test_table_checks_need_no_device():
    steps = [5, 3]
    tabs, nc = lf._checked_tables([np.ones(5), np.ones(2)], 2, steps, kept=False)
    assert nc == 1 and [t.shape for t in tabs] == [(5, 1), (2, 1)] and all(t.flags.c_contiguous for t in tabs)
    tabs, nc = lf._checked_tables([np.ones((5, 8)), np.ones((0, 8))], 2, steps, kept=True)
    assert nc == 8 and tabs[1].shape == (0, 8)
    with pytest.raises(ValueError, match="one coefficient table per column"):
        lf._checked_tables([np.ones(5)], 2, steps, kept=True)
    with pytest.raises(ValueError, match="one width"):
        lf._checked_tables([np.ones((5, 2)), np.ones((3, 1))], 2, steps, kept=True)
    with pytest.raises(ValueError, match="column 1: 4 coefficients but the run took 3 steps"):
        lf._checked_tables([np.ones(5), np.ones(4)], 2, steps, kept=True)
    # the product pass serves one or two combinations per column; wider tables need the kept basis
    for nc in (3, 4, 8):
        with pytest.raises(ValueError, match="NC = 1 or 2"):
            lf._checked_tables([np.ones((5, nc)), np.ones((3, nc))], 2, steps, kept=False)
        assert lf._checked_tables([np.ones((5, nc)), np.ones((3, nc))], 2, steps, kept=True)[1] == nc

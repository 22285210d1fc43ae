"""Device shifted MINRES (``csrc/minres_shifts.hip``) held to extended precision over its first K = 6 steps, and pinned on
shifts that stop while others go on (``_shifted_steps.py`` holds the reference, the measure, the cases and the reasoning;
``test_shifted_steps_cpu.py`` checks them without a GPU).

A step is read by calling the C entry with ``rtol = atol = 0`` and ``maxiter = k``: it returns every ``x_j`` at step k,
``info[j] == k`` and ``|tau_j|`` in the statistics.  Every deviation of ``x_j`` and ``|tau_j|`` from the ``longdouble`` run is
held to ``8 D`` (``STEPS ...`` lines under ``-s`` print the observed ratios).  The stop cases run with ``atol = target``."""
import ctypes as C
import warnings

import numpy as np
import pytest

import _hiprec as hp
import _shifted_steps as ss
from _sweep_cases import shifted_options
from eigensolvers_amd import _lib
from eigensolvers_amd.hip_vector import _ptr_table
from test_gpu_minres_steps import SMALL_WINDOWS, device_operator

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason="longdouble is no wider than double on this machine")]

BOUND = ss.BOUND
GROUPS = (tuple(range(8)), (8,))            # the 9 shifts as solve_shifts cuts them: 8 and then the ninth in a call of its own


# ---------------------------------------------------------------- reading steps
def call_entry(hip, H, case, group, maxiter, atol=0.0):
    """One call of ``hipeig_minres_shifts`` on the shifts ``group`` (indices into ``case.shifts``, at most 8) with
    ``rtol = 0``: ``xr`` / ``xi`` (lists of arrays), ``x`` (complex, shape ``(S, n)``), ``info``, ``its``, ``abstau``, ``itn``."""
    ctx, n = H.ctx, case.op.n
    zs = [complex(case.shifts[i]) for i in group]
    S = len(zs)
    assert 1 <= S <= 8
    b = hip.HipVector(case.b.copy(), ctx=ctx)
    re = [ctx.alloc(n) for _ in zs]
    im = [ctx.alloc(n) for _ in zs]
    rt, keep1 = _ptr_table(re)
    it, keep2 = _ptr_table(im)
    zr = (C.c_double * S)(*[z.real for z in zs])
    zi = (C.c_double * S)(*[z.imag for z in zs])
    info = (C.c_int * S)(*([-1] * S))
    st = (C.c_double * (4 * S))()
    _lib.call("hipeig_minres_shifts", ctx.handle, H.handle, float(case.sign), S, zr, zi, b._buf.ptr, rt, it, 0.0, float(atol),
              int(maxiter), info, st)
    xr = [hip.HipVector(r).array for r in re]
    xi = [hip.HipVector(i).array for i in im]
    return dict(xr=xr, xi=xi, x=np.array(xr) + 1j * np.array(xi), info=list(info), its=[int(st[4 * j]) for j in range(S)],
                abstau=[float(st[4 * j + 1]) for j in range(S)], itn=[int(st[4 * j + 2]) for j in range(S)])


def device_steps(hip, H, case, group):
    """Records of steps 1 .. K (or n, if smaller).  At ``k == n`` an exact ``beta_{n+1} = 0`` ends the run with ``tau = 0``
    and ``info == 0``; everywhere else the iteration limit is the stop."""
    out = []
    for k in range(1, case.nsteps + 1):
        rec = call_entry(hip, H, case, group, k)
        S = len(group)
        assert rec["its"] == [k] * S and rec["itn"] == [k] * S, (case.name, k, rec["its"], rec["itn"])
        assert all(i == k or (k == case.op.n and i == 0) for i in rec["info"]), (case.name, k, rec["info"])
        out.append(rec)
    return out


def check_steps(label, case, group, recs, ref):
    """Every deviation of every shift's ``x`` and ``|tau|`` is <= 8 D; a real shift's imaginary part is exactly zero and its
    real part is held as well.  Prints the largest ratio per quantity over shifts and steps."""
    worst = {}
    for k, rec in enumerate(recs, start=1):
        dev = ss.step_deviations(case, k, rec["x"], rec["abstau"], ref, shifts=group)
        for i, j in enumerate(group):
            if complex(case.shifts[j]).imag == 0.0:
                assert not rec["xi"][i].any(), (label, k, j)
                dev["x.re"] = max(dev.get("x.re", 0.0), ss.deviation(rec["xr"][i], ref[k - 1]["x"][j].real))
        for q, d in dev.items():
            if not d < worst.get(q, (-1.0, 0))[0]:
                worst[q] = (d, k)
    print(f"STEPS {label}: largest deviation / (8 D = {BOUND:g} u): "
          + ", ".join(f"{q} {d / BOUND:.3f} (step {k})" for q, (d, k) in worst.items()))
    bad = {q: v for q, v in worst.items() if not v[0] <= BOUND}
    assert not bad, (label, bad)


def run_case(hip, H, case, label, groups=GROUPS):
    ref = ss.reference(case)
    out = []
    for group in groups:
        recs = device_steps(hip, H, case, group)
        assert len(recs) == min(ss.K, case.op.n)
        check_steps(f"{label} shifts {group[0]}..{group[-1]}", case, group, recs, ref)
        out.append(recs)
    return out


# ---------------------------------------------------------------- steps
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_g1037_nine_shifts(hip, sign):
    """8 shifts and then the ninth, real, in a call of its own."""
    case = ss.CASES[f"g1037 sign={sign:+.0f}"]
    run_case(hip, device_operator(hip, "g1037"), case, case.name)


@pytest.mark.parametrize("name", ["dense1", "dense2", "g63", "g64", "g65"])
def test_small_n(hip, name):
    """n = 1, 2: one workgroup, ``n >> 1`` of 0 and 1, K limited to n, the Krylov space ending at step n; 63, 64, 65: around
    one wave, 63 and 65 with the odd tails of ``ms_kc_kernel`` and ``ms_update_kernel``."""
    for sign in (1.0, -1.0):
        case = ss.CASES[f"{name} sign={sign:+.0f}"]
        run_case(hip, device_operator(hip, name), case, case.name)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_n20001_every_sweep_layout(hip, variant):
    """Every sweep that carries ``LanczosRowEpilogue``; layouts 1 and 2 have more than 64 row blocks, so the two-level finish
    of the sweep's reduction runs."""
    case = ss.CASES["g20001 sign=+1" if variant & 1 else "g20001 sign=-1"]
    H = device_operator(hip, "g20001")
    H.set_variant(variant)
    run_case(hip, H, case, f"{case.name} layout {variant}")
    assert H.last_variant() == H.VARIANTS[variant]


def test_n20001_column_split_sweep(hip, monkeypatch):
    """The epilogue in the combine launch of a column-split blocked sweep: three shares per row block, 1 Ki-column windows."""
    for k, v in SMALL_WINDOWS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HIPEIG_TCOOW_CSPLIT", "3")
    case = ss.CASES["g20001 sign=+1"]
    H = device_operator(hip, "g20001", fresh=True)
    H.set_variant(4)
    run_case(hip, H, case, "g20001 layout 4 csplit=3")
    info = H.layout_info()
    assert info["column_splits"] == 3 and info["windows"] >= 3 and info["rows_per_block"] == 64, info


def test_n20001_small_grids(hip, monkeypatch):
    """One element per thread: 79 workgroups in ``ms_kc_kernel`` (the two-level finish of its reduction) and the largest
    grid of ``ms_update_kernel``."""
    monkeypatch.setenv("HIPEIG_MS_PER_THREAD", "1")
    monkeypatch.setenv("HIPEIG_MS_UPDATE_PER_THREAD", "1")
    case = ss.CASES["g20001 sign=-1"]
    run_case(hip, device_operator(hip, "g20001"), case, "g20001 per_thread=1 update_per_thread=1")


def _same_bits(a, b):
    assert a["info"] == b["info"] and a["its"] == b["its"] and a["itn"] == b["itn"] and a["abstau"] == b["abstau"]
    for p in ("xr", "xi"):
        for u, v in zip(a[p], b[p]):
            np.testing.assert_array_equal(u, v)


def test_g1037_chunk_of_one_step(hip, monkeypatch):
    """A look at the state record after every step against one after 32: every step record bit for bit the same (layout 2
    fixes the order of a row's adds), both within the bound."""
    case = ss.CASES["g1037 sign=+1"]
    H = device_operator(hip, "g1037")
    H.set_variant(2)
    monkeypatch.delenv("HIPEIG_MS_CHUNK", raising=False)
    default = run_case(hip, H, case, "g1037 layout 2 chunk=32")
    monkeypatch.setenv("HIPEIG_MS_CHUNK", "1")
    single = run_case(hip, H, case, "g1037 layout 2 chunk=1")
    for ga, gb in zip(default, single):
        for a, b in zip(ga, gb):
            _same_bits(a, b)
    assert H.last_variant() == H.VARIANTS[2]


# ---------------------------------------------------------------- stops
def _check_stops(label, case, rec, maxiter):
    """Every shift against the reference at the step it is expected to end at: its stop step, or ``maxiter`` while live."""
    ref = ss.reference(case)
    worst = {"x": 0.0, "tau": 0.0}
    for j, e in enumerate(case.expect):
        k = maxiter if e is None else e
        assert rec["its"][j] == k and rec["info"][j] == (maxiter if e is None else 0), (label, j, rec["its"], rec["info"])
        worst["x"] = max(worst["x"], ss.x_deviation(rec["x"][j], ref[k - 1]["x"][j]))       # touched once more: step k + 1
        worst["tau"] = max(worst["tau"], ss.tau_deviation(rec["abstau"][j], ref[k - 1]["abstau"][j]))
        if complex(case.shifts[j]).imag == 0.0:
            assert not rec["xi"][j].any(), (label, j)
    print(f"STEPS {label}: its {rec['its']}, largest deviation / (8 D = {BOUND:g} u): "
          + ", ".join(f"{q} {d / BOUND:.3f}" for q, d in worst.items()))
    assert max(worst.values()) <= BOUND, (label, worst)


def test_shifts_that_stop_while_others_go_on(hip, monkeypatch):
    """Four far shifts stop at steps 3, 4, 4 and 2 between contour shifts that are still live at ``maxiter = 6``."""
    case = ss.STOPS["mixed"]
    H = device_operator(hip, "g1037")
    H.set_variant(2)
    group = tuple(range(len(case.shifts)))
    monkeypatch.delenv("HIPEIG_MS_CHUNK", raising=False)
    rec = call_entry(hip, H, case, group, ss.K, atol=case.target)
    _check_stops("stops mixed chunk=32", case, rec, ss.K)
    assert rec["itn"] == [ss.K] * len(group)
    monkeypatch.setenv("HIPEIG_MS_CHUNK", "1")
    one = call_entry(hip, H, case, group, ss.K, atol=case.target)
    _check_stops("stops mixed chunk=1", case, one, ss.K)
    _same_bits(rec, one)


def test_every_shift_stops_before_the_limit(hip):
    """Eight far shifts, the last stop at step 4: the run ends by ``done`` before ``maxiter = 6``, through the C entry and
    through ``solve_shifts`` (no warning, ``products`` the slowest shift's steps)."""
    case = ss.STOPS["all-stop"]
    H = device_operator(hip, "g1037")
    last = max(case.expect)
    assert last < ss.K
    rec = call_entry(hip, H, case, tuple(range(8)), ss.K, atol=case.target)
    _check_stops("stops all", case, rec, ss.K)
    assert rec["itn"] == [last] * 8
    b = hip.HipVector(case.b.copy(), shifted_options(0.0, case.target, ss.K), ctx=H.ctx)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        xs = hip.solve_shifts(H, b, case.shifts)
    st = b.last_solve_stats
    assert st["iterations"] == case.expect and st["products"] == last
    ref = ss.reference(case)
    dev = [ss.x_deviation(x.array, ref[k - 1]["x"][j]) for j, (x, k) in enumerate(zip(xs, case.expect))]
    est = st["estimates"]
    ends = (int(np.argmax(est)), int(np.argmin(est)))
    tdev = [ss.tau_deviation(est[j], ref[case.expect[j] - 1]["abstau"][j]) for j in ends]
    print(f"STEPS stops all solve_shifts: x {max(dev) / BOUND:.3f}, estimates {est[ends[0]]:.3e} and {est[ends[1]]:.3e}: "
          f"{tdev[0] / BOUND:.3f}, {tdev[1] / BOUND:.3f} of 8 D")
    assert max(dev) <= BOUND and max(tdev) <= BOUND

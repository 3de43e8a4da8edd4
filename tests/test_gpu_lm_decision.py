"""The Levenberg-Marquardt decision kernels of the device-decided run -- reduce_report_kernel with lm_decide, lm_decide_failed_kernel,
lm_run_init_kernel, restore_if_rejected_kernel (csrc/ba_edge.hip) -- and the host's per-record logic (LmRun::absorb, csrc/ba_solver.hpp) run
on SCRIPTED sums through the hook cuba_hip_debug_lm_script (capi.lm_script), against the literal transliteration of the reference's loops
in tests/lm_decision_reference.py.  Both libraries.  Sums are handed over as partial arrays of small integers, so every order of summation
is exact in fp32 and fp64 and the decisions can be held to the reference BIT FOR BIT; the hook puts guard values around each array, so a
read outside it changes the total.

What ran on the MI355X (fp64 and fp32 library alike unless noted; `trials' = trials the reference runs, all of them absorbed by the host
logic, which stops at the last one; the scripts go on for three or more trials after that):

  script                  trials  iterations  the run ends on
  accepted_only                4           4  niter
  clamp_edges                  5           5  niter
  reject_then_accept           6           3  niter
  nine_then_accept            11           2  niter
  ten_rejections              10           1  the tenth rejection in a row (halt)
  six_accept_six_accept       15           3  niter
  zero_after_accept            2           2  rho == 0 (halt)
  zero_first_trial             1           1  rho == 0 (halt); empty partial arrays
  nan_fhat                     5           4  niter (two iterations end on a NaN gain ratio, no halt, nu goes on doubling)
  failed_mixed                 8           3  niter
  all_failed                  10           1  the tenth rejection in a row (halt)
  infinite_damping            10           1  the tenth rejection; see (*)
  niter0                       0           0  nothing absorbed, nothing written
  niter1_rejections            4           1  niter
  longer_than_the_ring        90          30  niter (tags checked through the ring's wrap at 64)
  beyond_float_range           7           3  niter; see (**)

  (*) the one allowed difference: the device halts at the seventh rejection, where the damping becomes infinite; trials 8 to 10 of that
  iteration are void on the device (rejected whatever they computed: F, damping and nu stay, the scratch estimate is restored) where the
  reference runs them with an infinite damping.  The host logic counts them as rejections all the same: one iteration, chi2 = [F0], final
  damping +inf, stop at the tenth trial -- the reference's.

  (**) fp32 library, damping beyond FLT_MAX while the double stays finite (1e38 -> 2e38 -> 8e38 -> 6.4e39 -> 4.3e39 -> ...): the decision
  goes on in double exactly as in the fp64 library (every record bit-equal to the reference's), and from the second rejection on the
  kernels are handed +inf as the damping (the `Scalar' slot reads 2e38, then inf for the remaining five trials).  The run ends as the
  reference's loop ends it (niter here).  The reference built with USE_FLOAT32 does the same: its optimize() keeps lambda in a double and
  setLambda() hands the kernels ScalarCast(lambda) = +inf.  No difference, nothing to fix.  (infinite_damping in the fp32 library: the
  kernels read +inf from the start, 1e300 being beyond float range; the decisions are the fp64 library's.)

  sums (three arrays of different lengths per launch, parts 1 + i % 7): lengths 0, 1, 63, 64, 65, 1023, 1024, 1025, 3071, 3072, 3073, 4095,
  4096, 4097, 7168, 7169, 8193 -- every total EXACT on both libraries.  Non-integers over twelve decades with one negative part (lengths
  5000, 4097, 1025), held to the bound n * u * sum|x| against math.fsum: worst error seen 0 in fp64 (the three totals are the correctly
  rounded sums; a CPU restatement of the kernel's order gives the same), 2.9e-4 of the bound in fp32 (4.7 against 5.0e4 at n = 5000)."""
import math

import numpy as np
import pytest

from lm_decision_reference import SCRIPTS, reference_run

from cuba_amd.capi import lm_script

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 3071, 3072, 3073, 4095, 4096, 4097, 7168, 7169, 8193)
TAG_BASE = 65536.0 * 7
EXTRA = [(1, 1, 600, 400)] * 3            # tempting trials behind every script: Fhat = 1 would be accepted wherever F > 1


@pytest.fixture(params=["f64", "f32"])
def precision(request):
    return request.param


def _same(a, b):
    return a == b or (a != a and b != b)


def _scalar(x, precision):
    if precision == "f64":
        return float(x)
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def _parts(total, n):
    """n small integers that add up to `total` (an integer-valued float below 2^24, or NaN: one NaN part); n = 0 for total 0 only"""
    if total != total:
        p = 1.0 + np.arange(max(n, 1)) % 7
        p[len(p) // 2] = float("nan")
        return p
    assert total == int(total) and abs(total) < 2 ** 23
    if n == 0:
        assert total == 0
        return np.zeros(0)
    p = 1.0 + np.arange(n) % 7
    p[-1] = total - p[:-1].sum()
    assert p.sum() == total and np.abs(p).sum() < 2 ** 24
    return p


def _hook_trials(trials):
    ns = (1, 5, 64, 65, 130, 1025, 3073, 4097)
    out = []
    for k, (ok, Fhat, sumLm, sumPose) in enumerate(trials):
        if not ok:
            out.append((0, None, None, None))
            continue
        zero = Fhat == 0 and sumLm == 0 and sumPose == 0
        out.append((1, _parts(sumLm, 0 if zero else ns[k % 8]), _parts(Fhat, 0 if zero else ns[(k + 3) % 8]), _parts(sumPose, 0 if zero else ns[(k + 5) % 8])))
    return out


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_decisions_follow_the_reference(name, precision):
    """every script, trial by trial: record and state bit-equal to the reference's, the `Scalar' damping its rounding, the scratch estimate
    restored after a rejection and only then; the host logic's chi2 series, iteration count, final F and damping, and the trial at which it
    stops; after a halt every further trial is void"""
    F0, lam0, niter, script = SCRIPTS[name]
    script = list(script) + EXTRA
    want = reference_run(F0, lam0, niter, script)
    used, recs = want["used"], want["records"]
    start, got = lm_script(_hook_trials(script), niter, F0=F0, lam0=lam0, tag_base=TAG_BASE, scratch_count=300, precision=precision)
    assert start["state"] == dict(F=F0, lam=lam0, nu=2.0, halt=0.0, trials=0.0, accepted=1.0, rej=0.0, maxq=10.0, tag_base=TAG_BASE)
    assert start["lam_scalar"] == _scalar(lam0, precision)
    # (the allowed difference: from the trial after the one whose damping overflowed, the device's trials are void)
    inf_at = next((k for k, r in enumerate(recs) if not math.isfinite(r["lam"])), None)
    halts = want["ended"] != "niter" or inf_at is not None
    halt_at = (inf_at if inf_at is not None else used - 1) if halts else None
    for k in range(used):
        g, r, s = got[k], recs[k], script[k]
        label = (name, precision, k, g, r)
        assert g["state"]["trials"] == k + 1 and g["record"]["tag"] == TAG_BASE + k + 1, label
        assert g["absorbed"] == 1, label
        if s[0]:
            assert g["sums"] == (s[2], s[1], s[3]) or s[1] != s[1], label
            assert g["slots_zero"], label
            assert _same(g["record"]["Fhat"], float(s[1])) and g["record"]["scale"] == (s[2] + s[3]) + 1e-3, label
        else:
            assert g["sums"] is None and g["record"]["Fhat"] == 0.0 and g["record"]["scale"] == 1e-3 and g["record"]["rho"] == -1.0, label
        if halt_at is not None and k > halt_at:
            continue                                  # (void trials: checked below)
        assert _same(g["record"]["rho"], r["rho"]), label
        assert g["record"]["lam"] == r["lam"] == g["state"]["lam"] and g["record"]["F"] == r["F"] == g["state"]["F"], label
        assert (g["record"]["accepted"] == 1.0) == r["accepted"] == (g["state"]["accepted"] == 1.0), label
        assert g["state"]["nu"] == r["nu"] and g["state"]["rej"] == r["rej"], label
        assert g["lam_scalar"] == _scalar(r["lam"], precision), label
        assert g["restored"] == (not r["accepted"]) and g["untouched"] == r["accepted"], label
        assert g["record"]["halt"] == g["state"]["halt"] == (1.0 if k == halt_at else 0.0), label
        last_of_iteration = k == used - 1 or recs[k + 1]["iteration"] != r["iteration"]
        assert g["rej_run"] == (0 if last_of_iteration else r["rej"]) and (g["chi2"] is not None) == last_of_iteration, label
    if halt_at is not None:
        h = got[halt_at]
        for k in range(halt_at + 1, len(script)):
            g = got[k]
            label = (name, precision, k, g)
            assert g["record"]["accepted"] == 0.0 and g["state"]["accepted"] == 0.0 and g["record"]["halt"] == 1.0 == g["state"]["halt"], label
            assert _same(g["state"]["F"], h["state"]["F"]) and g["state"]["lam"] == h["state"]["lam"] and g["state"]["nu"] == h["state"]["nu"], label
            assert g["record"]["lam"] == h["state"]["lam"] and g["record"]["F"] == h["state"]["F"], label
            assert g["lam_scalar"] == h["lam_scalar"] and g["restored"] and not g["untouched"], label
            assert g["state"]["trials"] == k + 1 and g["record"]["tag"] == TAG_BASE + k + 1, label
    # device + host logic together: the reference's run
    chi2 = [g["chi2"] for g in got if g["chi2"] is not None]
    assert chi2 == want["chi2"], (name, chi2, want["chi2"])
    stops = [k for k, g in enumerate(got) if g["stop"]]
    final = got[-1]
    if niter == 0:
        assert stops[0] == 0 and all(g["absorbed"] == 0 for g in got) and final["done"] == 0 and final["host_lam"] == lam0 and final["host_F"] == F0
        # (the device decides what it is fed all the same)
        assert got[0]["state"]["trials"] == 1.0
    else:
        assert stops[0] == used - 1, (name, stops, used)
        assert all(g["absorbed"] == 0 for g in got[used:])
        assert final["done"] == len(want["chi2"]) and final["host_F"] == want["F"] and _same(final["host_lam"], want["lam"]), (name, final, want["lam"])
    print(f"\n[lm script] {name} {precision}: {used} trials, {len(want['chi2'])} iterations, ends on {want['ended']}"
          + (f", device halt at trial {halt_at + 1}" if halt_at is not None else "")
          + f", damping handed to the kernels {[g['lam_scalar'] for g in got[:used]][:8]}")


def test_sums_are_exact_at_every_boundary(precision):
    """parts 1 + i % 7 at the boundaries of the 1024-thread, 4-way unrolled share (i + 3072 < n), three different lengths per launch: the
    slot totals EQUAL the integer sums, the groups' other slots are zero"""
    n = len(LENGTHS)
    trials, want = [], []
    for k in range(n):
        ls = (LENGTHS[k], LENGTHS[(k + 5) % n], LENGTHS[(k + 11) % n])
        arrs = [1.0 + np.arange(m) % 7 for m in ls]
        trials.append((1, *arrs))
        want.append(tuple(float(a.sum()) for a in arrs))
    _, got = lm_script(trials, 1, F0=1.0, lam0=1.0, precision=precision)
    for k in range(n):
        assert got[k]["sums"] == want[k] and got[k]["slots_zero"], (precision, k, LENGTHS[k], got[k]["sums"], want[k])
        assert got[k]["record"]["Fhat"] == want[k][1] and got[k]["record"]["scale"] == (want[k][0] + want[k][2]) + 1e-3


def test_sums_of_non_integers(precision):
    """values over twelve decades, one part negative: |sum - fsum| <= n * u * sum|x|, the bound of ANY order of summation"""
    rng = np.random.default_rng(11)
    u = 2.0 ** -53 if precision == "f64" else 2.0 ** -24
    arrs = []
    for m in (5000, 4097, 1025):
        x = 10.0 ** rng.uniform(-6, 6, m)
        x[17] = -x[17]
        if precision == "f32":
            x = x.astype(np.float32).astype(np.float64)          # (what the hook hands the kernels)
        arrs.append(x)
    _, got = lm_script([(1, *arrs)], 1, F0=1.0, lam0=1.0, precision=precision)
    worst = 0.0
    for x, s in zip(arrs, got[0]["sums"]):
        exact, bound = math.fsum(x.tolist()), len(x) * u * math.fsum(np.abs(x).tolist())
        worst = max(worst, abs(s - exact) / bound)
        print(f"\n[lm sums] {precision} n {len(x)}: |sum - fsum| {abs(s - exact):.3e}, bound {bound:.3e}")
        assert abs(s - exact) <= bound, (precision, len(x), s, exact, bound)
    print(f"[lm sums] {precision}: worst error {worst:.2e} of the bound")


@pytest.mark.parametrize("where", ["first", "last", "tied", "all_zero"])
def test_run_start_on_the_device(where, precision):
    """lm_run_init_kernel: F0 the slot-by-slot sum, the damping tau * the largest of the 64 patterns, the state as the host branch of
    lmRunBegin writes it; and the run that follows decides as the reference"""
    rng = np.random.default_rng(3)
    slots = rng.uniform(0.5, 900.0, 16)
    if precision == "f32":
        slots = slots.astype(np.float32).astype(np.float64)
    F0 = 0.0
    for v in slots.tolist():
        F0 += v
    diag = rng.uniform(1.0, 5e4, 64)
    big = 7.25e5 + 1.0 / 3
    if where == "first":
        diag[0] = big
    elif where == "last":
        diag[63] = big
    elif where == "tied":
        diag[5] = diag[40] = big
    else:
        diag[:] = 0.0
    lam0 = 1e-5 * float(diag.max())
    script = [(1, 2 * 10 ** 6, 50, 50), (1, 1000, 600, 400)]         # (a rejection, then an accept: F0 is below 16 * 900)
    start, got = lm_script(_hook_trials(script), 1, chi_slots=slots, maxdiag_bits=diag.view(np.uint64), tau=1e-5, tag_base=TAG_BASE, precision=precision)
    host_start, _ = lm_script([], 1, F0=F0, lam0=lam0, tag_base=TAG_BASE, precision=precision)
    assert start == host_start, (start, host_start)
    assert start["state"] == dict(F=F0, lam=lam0, nu=2.0, halt=0.0, trials=0.0, accepted=1.0, rej=0.0, maxq=10.0, tag_base=TAG_BASE)
    assert start["lam_scalar"] == _scalar(lam0, precision)
    want = reference_run(F0, lam0, 1, script)
    for g, r in zip(got, want["records"]):
        assert _same(g["record"]["rho"], r["rho"]) and g["record"]["lam"] == r["lam"] and g["record"]["F"] == r["F"], (where, g, r)
        assert (g["record"]["accepted"] == 1.0) == r["accepted"]
    assert want["used"] == 2 and got[1]["stop"] and got[1]["chi2"] == 1000.0


@pytest.mark.parametrize("count", [1, 255, 256, 257, 512 * 256 + 1])
def test_restore_if_rejected(count, precision):
    """state == backup after a rejected trial (failed solve, rho < 0, rho == 0 -> halt, a void trial) and untouched after an accepted one,
    at one number, around one workgroup, and past the 512-workgroup cap of the grid"""
    script = [(0, 0, 0, 0), (1, 900, 60, 40), (1, 950, 50, 50), (1, 800, 50, 50), (1, 800, 50, 50), (1, 100, 50, 50)]
    want = reference_run(1000.0, 1.0, 6, script)
    assert [r["accepted"] for r in want["records"]] == [False, True, False, True, False] and want["ended"] == "rho<=0"
    _, got = lm_script(_hook_trials(script), 6, F0=1000.0, lam0=1.0, scratch_count=count, precision=precision)
    for g, acc in zip(got, [False, True, False, True, False, False]):
        assert g["restored"] == (not acc) and g["untouched"] == acc and (g["state"]["accepted"] == 1.0) == acc, (count, g)


def test_the_hook_checks_its_arguments():
    """lengths, counts and pointers that could fault never reach a launch"""
    import ctypes as C
    from cuba_amd import capi
    lib = capi.load_library("f64")
    start, out = np.zeros(10), np.zeros(32 * 4)
    ok = np.ones(2, dtype=np.int32)
    good, a = np.array([0, 1, 2], dtype=np.int32), np.ones(4)

    def call(niter=1, n=2, ok=ok, a=a, a_off=good, b_off=good, c_off=good, scratch=1, start=start, out=out, mode=0, tag=0.0):
        return lib.cuba_hip_debug_lm_script(0, mode, 1.0, 1.0, None, None, 1e-5, tag, niter, n, capi._i(ok), capi._d(a), capi._i(a_off), capi._d(a), capi._i(b_off),
                                            capi._d(a), capi._i(c_off), scratch, capi._d(start), capi._d(out))
    assert call() == 0
    bad = [dict(n=-1), dict(n=513), dict(niter=-1), dict(niter=513), dict(ok=None), dict(a_off=None), dict(start=None), dict(out=None),
           dict(a=None), dict(a_off=np.array([1, 1, 2], dtype=np.int32)), dict(b_off=np.array([0, 2, 1], dtype=np.int32)),
           dict(c_off=np.array([0, 1, 70000], dtype=np.int32)), dict(scratch=2 ** 20 + 1), dict(mode=1), dict(mode=2), dict(tag=-1.0),
           dict(tag=float("nan"))]
    for kw in bad:
        assert call(**kw) == 1, kw
    n = C.c_size_t()
    assert lib.cuba_hip_debug_lm_records(None, None, 0, C.byref(n)) != 0

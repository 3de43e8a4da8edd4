"""The edge-gating reference (tests/edge_gate_reference.py) against the oracle, and the zero-information oracle -- an OracleSolver on the
graph with the gated edges' information set to 0 -- as the reference of a gated handle: it agrees with an OracleSolver on the graph with
those edges removed.  Then the figures of the 5 + 10 flow on the suite's small graph, which the GPU tests repeat on the device."""
import numpy as np
import pytest

import edge_gate_reference as R
from conftest import RK_HUBER
from oracle.oracle import OracleSolver


@pytest.fixture(scope="module")
def flow(small_fp):
    """optimize(5), gate, optimize(10) on the zero-information oracle, reclassify"""
    o = OracleSolver(small_fp, RK_HUBER)
    start = R.classify(small_fp)
    chi_start = o.chi_squares()
    o.optimize(5)
    s5 = o.state()
    chi5 = o.chi_squares()
    c5 = R.classify(small_fp, s5)
    z = OracleSolver(R.with_state(R.zero_information(small_fp, c5["mask"]), s5), RK_HUBER)
    run = z.optimize(10)
    c15 = R.classify(small_fp, z.state(), prev=c5["mask"])
    return dict(start=start, chi_start=chi_start, s5=s5, chi5=chi5, c5=c5, run=run, c15=c15)


def test_reference_chi2_equals_the_oracles(small_fp, flow):
    for got, want in ((flow["start"]["chi2"], flow["chi_start"]), (flow["c5"]["chi2"], flow["chi5"])):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(want, 1.0))


def test_zero_information_equals_removed_edges(small_fp):
    mask = R.mask_keeping_two_per_landmark(small_fp, np.random.default_rng(7))
    assert 200 < (~mask).sum() and R.landmark_counts(small_fp, mask).min() >= 2
    zero = OracleSolver(R.zero_information(small_fp, mask), RK_HUBER).optimize(8)["chi2"]
    gone = OracleSolver(R.without_edges(small_fp, mask), RK_HUBER).optimize(8)["chi2"]
    assert len(zero) == len(gone) == 8
    assert np.all(np.abs(zero - gone) <= 1e-9 * gone), np.abs(zero - gone) / gone


def test_figures_of_the_flow_on_the_small_graph(small_fp, flow):
    fp, start, c5, c15 = small_fp, flow["start"], flow["c5"], flow["c15"]
    assert (~start["mask"]).sum() == 2034 and start["depth"].min() == pytest.approx(4.09, abs=0.005)
    assert start["counts"] == dict(active_mono=50, active_stereo=316, gated_chi2_mono=293, gated_chi2_stereo=1741, gated_depth=0, changed=2034)
    assert c5["counts"] == dict(active_mono=328, active_stereo=1945, gated_chi2_mono=15, gated_chi2_stereo=112, gated_depth=0, changed=127)
    assert (c5["per_landmark"] < 2).sum() == 14 and (c5["per_landmark"] == 0).sum() == 6
    assert flow["run"]["chi2"][0] == pytest.approx(4185.5, abs=0.05) and flow["run"]["chi2"][-1] == pytest.approx(3884.7, abs=0.05)
    assert (c15["mask"] & ~c5["mask"]).sum() == 5 and (~c15["mask"] & c5["mask"]).sum() == 3 and c15["counts"]["changed"] == 8
    # no decision hangs on rounding: the nearest edge is 7.3e-4 / 3.1e-4 (relative) from its threshold
    assert R.threshold_margin(fp, start["chi2"]).min() > 1e-6 and R.threshold_margin(fp, c5["chi2"]).min() > 1e-6
    for c, (n3, n2) in ((start, (3, 7)), (c5, (1, 6))):
        m = R.threshold_margin(fp, c["chi2"])
        assert ((m < 1e-3).sum(), (m < 1e-2).sum()) == (n3, n2)


def test_modes_and_depth_of_the_reference(small_fp, flow):
    fp, c5 = small_fp, flow["c5"]
    cd = (c5["chi2"], c5["depth"])
    prev = np.ones(fp.E, bool); prev[np.flatnonzero(c5["mask"])[:20]] = False
    only = R.classify(fp, prev=prev, mode="only_remove", chi_depth=cd)
    assert not (only["mask"] & ~prev).any() and np.array_equal(only["mask"], c5["mask"] & prev)
    dry = R.classify(fp, prev=prev, mode="dry_run", chi_depth=cd)
    assert np.array_equal(dry["mask"], prev) and dry["counts"]["changed"] == (c5["mask"] != prev).sum()
    # depth: a point behind its camera is gated by depth whatever its chi2; a NaN fails both tests
    depth = c5["depth"].copy(); depth[:3] = -1.0; depth[3] = 0.0
    chi = c5["chi2"].copy(); chi[4] = np.nan
    d = R.classify(fp, chi_depth=(chi, depth))
    assert not d["mask"][:5].any() and d["counts"]["gated_depth"] == 4
    assert R.classify(fp, chi_depth=(chi, depth), positive_depth=False)["counts"]["gated_depth"] == 0
    assert R.classify(fp, chi_depth=(chi, depth), chi2_max=(np.inf, np.inf), positive_depth=False)["mask"].sum() == fp.E - 1

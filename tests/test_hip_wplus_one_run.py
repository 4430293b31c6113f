"""The W+ loop has ONE definition of a step (engine._WRun._eager_step) and three ways to run it: launch by launch from Python, replayed
from a launch plan, replayed from a captured hipGraph.  Pinned here:

  * against the commit before the graph replay became a replay kind of ``_WRun`` (tests/golden/wplus_one_run_parent.npz, recorded on the
    MI355X by tests/golden/make_wplus_one_run_parent.py; tests/wplus_one_run_cases.py lists the cases): equal loss bits, equal SHA-256 of
    the latents, equal ``last_stats`` and equal dispatch counters — every conv went to the same kernel family as often as before, the
    arithmetic and its order did not move;
  * between the three kinds, whatever the commit: bit-equal latents and losses, and what ``last_plan`` reports for each;
  * a graph run whose range flag is raised mid-run is repeated as a whole through the guarded loop;
  * ``GeneratorEngine.clone_shared()`` shares the prepared data and nothing of the per-run state."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wplus_one_run_cases as WC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wplus_one_run_parent.npz')


@pytest.fixture(scope='module')
def parent():
    return np.load(GOLDEN)


@pytest.fixture
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', list(WC.CASES))
def test_bits_stats_and_dispatch_of_the_parent_commit(parent, dev, name):
    assert tuple(str(c) for c in parent['counter_names']) == WC.COUNTERS
    bad = []
    for mode, rec in WC.record(name, dev).items():
        for k, v in rec.items():
            want = parent[f'{name}/{mode}/{k}']
            same = v.shape == want.shape and np.array_equal(v, want)
            print(f'{name} {WC.CASES[name]} {mode} {k}: {"equal" if same else f"{v.tolist()} != parent {want.tolist()}"}')
            if not same:
                bad.append((mode, k))
    assert not bad, bad


def test_three_replay_kinds_are_bit_identical(dev):
    size, B, streams, steps = WC.CASES['s64_b3']
    eng, target, noises, w0 = WC.inputs(size, B, dev)
    res = {mode: WC.run_mode(eng, target, noises, w0, streams, steps, mode) for mode in WC.MODES}
    (ig, wg, lg, _), (ip, wp, lp, _), (ie, we, le, _) = res['graph'], res['plan'], res['python']
    assert torch.equal(wg, wp) and torch.equal(lg, lp)
    assert torch.equal(wp, we) and torch.equal(lp, le)
    print(f'last_plan: graph {ig.last_plan}, plan {ip.last_plan}, python {ie.last_plan}')
    # the graph: step 1 from Python, step 2 captured (and replayed once to run it), the rest replayed; no launch of a launch plan
    assert ig.last_plan['steps'] == [steps - 2] and ig.last_plan['launches'] == [0]
    assert ip.last_plan['steps'] == [steps - 3]
    for inv in (ig, ip, ie):
        assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}


def test_graph_run_with_a_range_violation_is_repeated_whole(dev):
    """A graph run has no per-window guard: the flags are read once at its end and a flagged inversion is repeated, undisturbed, through
    the guarded loop — the result is that loop's, bit for bit."""
    from oodgan.engine import WPlusInverter
    size, B, steps = 32, 2, 12
    eng, target, noises, w0 = WC.inputs(size, B, dev)
    inv = WPlusInverter(eng)
    w_ref, l_ref = inv.invert(target, w0, noises, steps=steps)
    assert inv.last_stats == {'steps_run': [steps], 'rollbacks': [0]}
    done = []

    def sabotage(run):
        if run.steps_run == 5 and not done:
            done.append(run)
            assert eng.carry_range and eng.fused_bwd
            eng.fwd_range.q[3].mul_(2.0 ** 12)
    inv.on_step = sabotage
    w, l = inv.invert(target, w0, noises, steps=steps, use_graph=True)
    inv.on_step = None
    torch.cuda.synchronize()
    print(f'graph run, forward scale sabotaged after step 5 of {steps}: {inv.last_stats}, plan {inv.last_plan}')
    assert len(done) == 1 and done[0].replay == 'graph'     # the sabotaged run was the graph run
    assert inv.last_plan['steps'] == [steps - 3]        # ... and the one that returned the repeat through the launch plan
    assert torch.equal(w, w_ref) and torch.equal(l, l_ref)
    assert inv.last_stats['rollbacks'] == [0]
    assert eng.carry_range and eng.fused_bwd


@pytest.mark.parametrize('mode', list(WC.MODES))
def test_inverter_is_freed_when_dropped(dev, mode):
    """The inverter keeps the captured graphs (and their private pools) until its next call, so it must die by reference count when it is
    dropped: as part of a reference cycle (its runs point back to it) it would be freed whenever the collector happens to run — inside
    the next inverter's stream capture, where destroying a graph is not allowed."""
    import gc
    import weakref
    size, B, streams, steps = WC.CASES['s32_b2']
    eng, target, noises, w0 = WC.inputs(size, B, dev)
    inv, w, losses, _ = WC.run_mode(eng, target, noises, w0, streams, steps, mode)
    assert len(inv._graphs) == (1 if mode == 'graph' else 0)        # kept: replays may be in flight when invert returns
    ref = weakref.ref(inv)
    gc.collect()
    gc.disable()
    try:
        del inv
        assert ref() is None
    finally:
        gc.enable()


def test_clone_shared_shares_prepared_data_only(dev):
    eng, _, _, _ = WC.inputs(32, 1, dev)
    # an engine in use (no kernel needed to say so): every piece of per-run state holds something
    eng.saved, eng._fwd_serial, eng.last_gs = {'serial': 3}, 3, torch.zeros(1)
    eng.bwd_state['conv1'], eng.bwd_flag = torch.ones(2), torch.zeros(1, dtype=torch.int32)
    eng.fwd_range = eng._ranges[1] = object()
    c = eng.clone_shared()
    for name in ('bwd_state', '_ranges', 'saved'):
        assert getattr(c, name) is not getattr(eng, name), name
    assert c.bwd_state == {} and c._ranges == {} and c.saved is None and c.bwd_flag is None and c.fwd_range is None
    assert c._fwd_serial == 0 and c.last_gs is None
    assert eng.saved == {'serial': 3} and len(eng.bwd_state) == 1 and len(eng._ranges) == 1      # the original keeps its own
    assert c._const_b is eng._const_b
    assert c.wcat is eng.wcat and c.layers is eng.layers

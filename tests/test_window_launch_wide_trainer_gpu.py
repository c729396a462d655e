"""GPU: args.window_launch_wide — with args.window_launch, the Trainer plays the recorded rollout of a native update at hid 256 as ONE
launch per window (Trainer._play_window -> step_env_window / step_env_commnet_window -> ic3_policy_step on a descriptor tagged
IC3_POLICY_WINDOW_WIDE / IC3_COMMNET_WINDOW_WIDE) — against the per-step path of the same tree.

One train_batch of two windows from one seed with window_launch off, a second one with it off, one with window_launch and
window_launch_wide set.  The batch, the episode records (the state record, gates, the inp rows — H wide at this size —, log-prob rows,
snapshots, masks, counters) and the statistics must be equal bit for bit; the window counter is the number of windows and the
per-step counter is 0; every parameter gradient matches switch-off within 4 x the largest relative difference between the TWO
switch-off updates, measured in the run itself, with the figure recorded from the GPU in profiles/r24/window_launch_wide_errors.txt
as a floor under it (IC3_WINDOW_ERRORS=<file> appends a run's figures) — where both are 0, equality.  The floor comes from switch-off
pairs only.  One case runs in collection mode (auto_reset with window_launch_collection): the second window continues the streams.

What stays on the per-step path at hid 256 whatever the flags say: IRIC with the LSTM cell (no gate record there), comm_passes 2."""
import os

import pytest
import torch

from test_collection_window_launch_trainer_gpu import _count, _record
from test_window_launch_trainer_gpu import _copy, _equal, _rel_diff

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS, WINDOWS, HID = 8, 12, 2, 256

# (workload, flags, the per-step counter's family, collection mode)
_PP = dict(nagents=3, dim=5, vision=1, hid_size=HID, max_steps=T_STEPS)
CASES = {
    'pp_ic3net_h256': ('pp_easy', dict(nagents=3, dim=5, vision=0, hid_size=HID, max_steps=T_STEPS, detach_gap=4), 'mega', False),
    'tj_easy_h256': ('tj_easy_window_h256', dict(), 'mega', False),
    'pp_ic_h256': ('pp_hard_ic', dict(_PP), 'commnet', False),
    'pp_iric_tanh_h256': ('pp_hard_iric_tanh', dict(_PP, detach_gap=4), 'commnet', False),
    'tj_easy_commnet_h256_p2': ('tj_easy_commnet_window_h256', dict(), 'commnet', False),
    # collection mode on a 2 x 2 grid: predators meet the prey and episodes end well before max_steps, the streams leave the window
    # boundaries; the second window continues them
    'pp_ic3net_h256_collection': ('pp_easy', dict(nagents=3, dim=2, vision=0, hid_size=HID, max_steps=T_STEPS, detach_gap=4), 'mega', True),
}
# what keeps one launch per step at hid 256 with both flags set
PER_STEP = {
    'pp_iric_lstm_h256': ('pp_hard_iric', dict(_PP, detach_gap=4), 'mega', False),
    'pp_ic3net_h256_p2': ('pp_easy', dict(nagents=3, dim=5, vision=0, hid_size=HID, max_steps=T_STEPS, detach_gap=4, comm_passes=2), 'mega',
                          False),
}

# largest relative gradient difference between two switch-off updates from the seed, per case, as measured on the GPU
# (profiles/r24/window_launch_wide_errors.txt, the larger of the runs' figures; the encoder backward's expand stage adds with float
# atomics where two agents of an env share a window cell — their order moves the sums by an ulp or two of the largest entry)
NOISE_MEASURED = {'pp_ic3net_h256': 0.0, 'tj_easy_h256': 1.289e-07, 'pp_ic_h256': 0.0, 'pp_iric_tanh_h256': 9.089e-08,
                  'tj_easy_commnet_h256_p2': 0.0, 'pp_ic3net_h256_collection': 0.0}


def _build(case, on):
    import bench
    tj = dict(nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=HID, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3)
    bench.WORKLOADS.setdefault('tj_easy_window_h256', ("traffic_junction", dict(tj, ic3net=True, recurrent=True, detach_gap=4)))
    bench.WORKLOADS.setdefault('tj_easy_commnet_window_h256', ("traffic_junction", dict(tj, commnet=True, recurrent=False, comm_passes=2)))
    wl, flags, _, collection = dict(CASES, **PER_STEP)[case]
    tr, a = bench.build_trainer(wl, E_ENVS, 5, 0, 0, **flags)
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=WINDOWS * E_ENVS * a.max_steps)
    assert a.hid_size == HID
    a.auto_reset = collection
    a.window_launch = bool(on)
    a.window_launch_wide = int(on)
    a.window_launch_collection = int(on and collection)
    return tr, a


def _update(case, on):
    """One train_batch; returns what it rolled out (batch, records), its stat, every gradient and the counters."""
    tr, a = _build(case, on)
    cap = {}
    inner = tr.compute_grad_native
    lstm = bool(a.recurrent) and a.rnn_type == 'LSTM'

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        cap['records'] = [_record(r, lstm) for r in records]
        cap['xh_width'] = [r.xh.shape[2] if r.xh is not None else None for r in records]
        return inner(batch, records)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    family = dict(CASES, **PER_STEP)[case][2]
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=getattr(net, 'window_launches', 0), steps=_count(net, 'mega_steps' if family == 'mega' else 'commnet_steps'))
    return cap


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_window_launch_update_equals_the_per_step_update(case):
    off, off2, on = _update(case, False), _update(case, False), _update(case, True)
    family, collection = CASES[case][2], CASES[case][3]
    assert len(off['records']) == len(on['records']) == WINDOWS
    assert off['windows'] == 0 and off['steps'] == WINDOWS * T_STEPS
    assert on['windows'] == WINDOWS and on['steps'] == 0, "the window launch did not play every window"
    assert all(r['n'] == r['out_n'] == T_STEPS for r in on['records'])
    if family == 'mega':                                           # the gate record, its inp rows H wide
        assert all(r['has_gates'] and r['gates_n'] == T_STEPS for r in on['records']) and on['xh_width'] == [HID] * WINDOWS
    if case == 'pp_ic_h256':
        assert all(r['h_fin'] is not None and r['h_fin_n'] == T_STEPS for r in on['records'])
    if collection:
        assert [(r['stream']['first'], r['stream']['last']) for r in on['records']] == [(True, False), (False, True)]
        done = torch.stack([m['done'] for m in off['batch'][8]]).reshape(WINDOWS, T_STEPS, E_ENVS)
        assert int(done[:, :T_STEPS - 1].any(1).any(0).sum()) >= 2, "the streams stay on the window boundaries"
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    noise, diff = _rel_diff(off2['grads'], off['grads']), _rel_diff(on['grads'], off['grads'])
    line = ("%-26s %d windows; largest relative gradient difference: two switch-off updates %.3e (%s), switch on vs off %.3e (%s)"
            % (case, WINDOWS, max(noise.values()), max(noise, key=noise.get), max(diff.values()), max(diff, key=diff.get)))
    print(line)
    path = os.environ.get("IC3_WINDOW_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    # The bar is 4 x this run's own switch-off pair, the recorded switch-off figure a floor under it (a run's pair can happen to be 0
    # where the sums do not repeat); where both are 0, equality.
    bar = 4 * max(max(noise.values()), NOISE_MEASURED[case])
    for k in diff:
        if bar == 0.0:
            assert torch.equal(on['grads'][k], off['grads'][k]), (k, diff[k])
        else:
            assert diff[k] <= bar, (k, diff[k], bar)


@pytest.mark.parametrize("case", sorted(PER_STEP))
def test_what_stays_on_the_per_step_path_at_hid_256(case):
    tr, a = _build(case, True)
    assert a.window_launch and a.window_launch_wide == 1
    tr.train_batch(0)
    net = tr.policy_net
    steps = _count(net, 'mega_steps')
    assert getattr(net, 'window_launches', 0) == 0 and steps > 0 and steps % T_STEPS == 0
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)


def test_window_launch_alone_keeps_hid_256_on_the_per_step_path():
    case = 'pp_ic_h256'
    tr, a = _build(case, True)
    a.window_launch_wide = 0
    tr.train_batch(0)
    assert getattr(tr.policy_net, 'window_launches', 0) == 0 and _count(tr.policy_net, 'commnet_steps') == WINDOWS * T_STEPS

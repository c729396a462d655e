"""GPU: args.passes_in_launch_wide — a hid-256 recurrent CommNet / IC3Net policy with comm_passes 2..4 runs every step of its rollout as
ONE launch (CommNetMLP.step_env -> ic3_policy.npasses at hid 256), and with args.window_launch and args.window_launch_wide beside it
the Trainer plays its recorded rollout as ONE launch per window (Trainer._play_window -> step_env_window -> ic3_policy_step on a
descriptor tagged IC3_POLICY_WINDOW_WIDE_PASSES) — against the path of the same tree with every flag off (comm_passes launches per
step).

One train_batch of two windows from one seed with the flags off, a second one with them off, one with them set.  The batch, the
episode records (the state record, log-prob rows, snapshots, masks, counters) and the statistics must be equal bit for bit; the window
counter is the number of windows and the per-step counter is 0; every parameter gradient matches switch-off within 4 x the largest
relative difference between the TWO switch-off updates, measured in the run itself, with the figure recorded from the GPU in
profiles/r25/passes_in_launch_wide_errors.txt as a floor under it (IC3_WINDOW_ERRORS=<file> appends a run's figures) — where both are
0, equality.  The floor comes from switch-off pairs only.  One case runs in collection mode (auto_reset with
window_launch_collection): the second window continues the streams.  With args.passes_in_launch_wide alone the update is the same
update again, on the per-step path: one launch per step, no window."""
import os

import pytest
import torch

from test_collection_window_launch_trainer_gpu import _count, _record
from test_window_launch_trainer_gpu import _copy, _equal, _rel_diff

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS, WINDOWS, HID = 8, 12, 2, 256

# (workload, flags, collection mode)
CASES = {
    'pp_ic3net_h256_p2': ('pp_easy', dict(nagents=3, dim=5, vision=0, hid_size=HID, max_steps=T_STEPS, detach_gap=4, comm_passes=2), False),
    'tj_easy_h256_p3_shared': ('tj_easy_window_h256', dict(comm_passes=3, share_weights=True), False),
    # collection mode on a 2 x 2 grid: predators meet the prey and episodes end well before max_steps, the streams leave the window
    # boundaries; the second window continues them (the update of its windows through the window backward, as the lock-step cases')
    'pp_ic3net_h256_p2_collection': ('pp_easy', dict(nagents=3, dim=2, vision=0, hid_size=HID, max_steps=T_STEPS, detach_gap=4,
                                                     comm_passes=2, multipass_window_collection=1), True),
}

# largest relative gradient difference between two switch-off updates from the seed, per case, as measured on the GPU
# (profiles/r25/passes_in_launch_wide_errors.txt, the larger of the runs' figures; the encoder backward's expand stage adds with float
# atomics where two agents of an env share a window cell — their order moves the sums by an ulp or two of the largest entry)
NOISE_MEASURED = {'pp_ic3net_h256_p2': 0.0, 'tj_easy_h256_p3_shared': 1.444e-07, 'pp_ic3net_h256_p2_collection': 0.0}


def _build(case, on, window=True):
    import bench
    tj = dict(nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=HID, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3)
    bench.WORKLOADS.setdefault('tj_easy_window_h256', ("traffic_junction", dict(tj, ic3net=True, recurrent=True, detach_gap=4)))
    wl, flags, collection = CASES[case]
    tr, a = bench.build_trainer(wl, E_ENVS, 5, 0, 0, **flags)
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=WINDOWS * E_ENVS * a.max_steps)
    assert a.hid_size == HID and a.comm_passes == flags['comm_passes']
    a.auto_reset = collection
    a.passes_in_launch_wide = int(on)
    a.window_launch = bool(on and window)
    a.window_launch_wide = int(on and window)
    a.window_launch_collection = int(on and window and collection)
    return tr, a


def _update(case, on, window=True):
    """One train_batch; returns what it rolled out (batch, records), its stat, every gradient and the counters."""
    tr, a = _build(case, on, window)
    cap = {}
    inner = tr.compute_grad_native

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        cap['records'] = [_record(r, True) for r in records]
        return inner(batch, records)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=getattr(net, 'window_launches', 0), steps=_count(net, 'mega_steps'))
    return cap


_OFF = {}


def _off(case):
    """The two switch-off updates of a case, shared by the tests that compare against them."""
    if case not in _OFF:
        _OFF[case] = (_update(case, False), _update(case, False))
    return _OFF[case]


def _compare(case, on, what):
    off, off2 = _off(case)
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    noise, diff = _rel_diff(off2['grads'], off['grads']), _rel_diff(on['grads'], off['grads'])
    line = ("%-30s %-13s %d windows; largest relative gradient difference: two switch-off updates %.3e (%s), switch on vs off %.3e (%s)"
            % (case, what, WINDOWS, max(noise.values()), max(noise, key=noise.get), max(diff.values()), max(diff, key=diff.get)))
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


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_update_with_every_flag_on_equals_the_update_with_them_off(case):
    off, _ = _off(case)
    on = _update(case, True)
    collection = CASES[case][2]
    assert len(off['records']) == len(on['records']) == WINDOWS
    assert off['windows'] == 0 and off['steps'] == WINDOWS * T_STEPS
    assert on['windows'] == WINDOWS and on['steps'] == 0, "the window launch did not play every window"
    assert all(r['n'] == r['out_n'] == T_STEPS and not r['has_gates'] for r in on['records'])
    if collection:
        assert [(r['stream']['first'], r['stream']['last']) for r in on['records']] == [(True, False), (False, True)]
        done = torch.stack([m['done'] for m in off['batch'][8]]).reshape(WINDOWS, T_STEPS, E_ENVS)
        assert int(done[:, :T_STEPS - 1].any(1).any(0).sum()) >= 2, "the streams stay on the window boundaries"
    _compare(case, on, "all flags")


def test_the_flag_alone_keeps_one_launch_per_step_and_the_same_update():
    case = 'pp_ic3net_h256_p2'
    on = _update(case, True, window=False)
    assert on['windows'] == 0 and on['steps'] == WINDOWS * T_STEPS
    _compare(case, on, "flag alone")


def test_the_window_flags_without_the_flag_keep_the_per_step_path():
    tr, a = _build('pp_ic3net_h256_p2', True)
    a.passes_in_launch_wide = 0
    tr.train_batch(0)
    assert getattr(tr.policy_net, 'window_launches', 0) == 0 and _count(tr.policy_net, 'mega_steps') == WINDOWS * T_STEPS

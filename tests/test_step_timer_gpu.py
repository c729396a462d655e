"""GPU: the step timer of the three one-launch rollout steps (raw.step_timer / step_timer_every / dispatch_events: what
bench.py reads its per-launch times from).  One eager episode with every second launch timed: the list holds exactly those
samples, every pair gives a time, and timing a launch changes nothing the rollout computes."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

E, T, EVERY = 7, 6, 2
SMALL_PP = dict(nagents=3, dim=5, vision=0)
CASES = {
    # the LSTM IC3Net / CommNet (ic3_policy_step)
    "lstm-pp": ("pp_easy", dict()),
    "lstm-tj": ("tj_medium", dict()),
    # the non-recurrent CommNet module, two communication passes (ic3_commnet_step)
    "commnet-pp": ("pp_easy", dict(ic3net=False, commnet=True, recurrent=False, comm_passes=2)),
    "commnet-tj": ("tj_medium_commnet_mlp", dict()),
    # models.RNN with the tanh recurrence (ic3_commnet_step with h_in)
    "rnn-pp": ("pp_hard_iric_tanh", dict(SMALL_PP)),
    "rnn-tj": ("tj_medium", dict(commnet=False, baseline='rnn', rnn_type='MLP')),
}


def _build(case):
    import bench
    wl, over = CASES[case]
    tr, a = bench.build_trainer(wl, E, 3, 20, 0, hid_size=64, max_steps=T, **over)
    return tr


def _play(case, timed, dispatch_events=False):
    tr = _build(case)
    raw = tr.env.env
    if timed:
        raw.step_timer = []
        raw.step_timer_every = EVERY
        raw.dispatch_events = dispatch_events
    episode, stat = tr.get_episode(0)
    torch.cuda.synchronize()
    assert len(episode) == T and tr._mega_last, "the one-launch path did not run"
    out = {k: tr._buf[k][:T].clone() for k in ('action', 'reward', 'done', 'alive', 'is_completed')}
    for t, (_, action_out, value, _) in enumerate(tr._step_out):
        for k, head in enumerate(action_out):
            out['action_out%d/%d' % (k, t)] = head.clone()
        out['value/%d' % t] = value.clone()
    return tr, raw, out


@functools.lru_cache(maxsize=None)
def _untimed(case):
    return _play(case, False)[2]


@pytest.mark.parametrize("case,dispatch_events", [(c, False) for c in CASES] + [("lstm-pp", True), ("lstm-tj", True)])
def test_every_second_launch_is_timed_and_the_rollout_is_unchanged(case, dispatch_events):
    from ic3net_amd.envs import DispatchEvent
    tr, raw, out = _play(case, True, dispatch_events)
    samples = raw.step_timer
    assert [s[2] for s in samples] == list(range(0, T, EVERY)) and all(len(s) == 3 for s in samples)
    # the LSTM step records torch events around the launch unless raw.dispatch_events; the other two always have the
    # dispatch stamp its own
    kind = DispatchEvent if dispatch_events or not case.startswith("lstm") else torch.cuda.Event
    for e0, e1, _ in samples:
        assert type(e0) is kind and type(e1) is kind
    step_all = [(s_.elapsed_time(e_), t_) for s_, e_, t_ in samples]           # (as bench.py reads them)
    for ms, t in step_all:
        assert math.isfinite(ms) and ms > 0.0, (t, ms)
    want = _untimed(case)
    assert set(out) == set(want)
    for k in want:
        assert out[k].dtype == want[k].dtype and torch.equal(out[k], want[k]), k

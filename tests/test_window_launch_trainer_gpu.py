"""GPU: args.window_launch — Trainer.get_episode plays the recorded rollout of a native update as ONE launch per window
(Trainer._play_window -> CommNetMLP.step_env_window -> ic3_policy_step on an ic3_policy_window) — against the per-step path of the
same tree: one train_batch from one seed with the switch off and one with it on.  The batch, the episode records (the (h, c) record,
gates, inp rows, log-prob rows, snapshots, masks, counters) and the statistics must be equal bit for bit; the window counter moves
and the per-step counter does not; every parameter gradient matches switch-off within 4 x the largest relative difference between
TWO switch-off updates from that seed (measured in the run itself and recorded in profiles/r20/window_launch_errors.txt, the larger
of the two; IC3_WINDOW_ERRORS=<file> appends a run's figures) — where that is 0, equality.  The fallbacks (store_states, collection mode, hid 256, a
window the library refuses) run the per-step path unchanged."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS = 8, 12

CASES = {
    'pp_ic3net_h64': ('pp_easy', dict(nagents=3, dim=5, vision=0, hid_size=64, max_steps=T_STEPS, detach_gap=4)),
    'tj_easy_h128': ('tj_easy_window', dict()),
    'pp_iric_lstm_h64': ('pp_hard_iric', dict(nagents=3, dim=5, vision=1, hid_size=64, max_steps=T_STEPS, detach_gap=4)),
}


# largest relative gradient difference between two switch-off updates from the seed, per case, as measured
# (profiles/r20/window_launch_errors.txt: the larger of the visits' figures; the encoder's expand stage adds with float atomics, whose
# order moves the sums by an ulp or two of the largest entry from run to run — 0 where no two agents of an env share a window cell)
NOISE_MEASURED = {'pp_ic3net_h64': 0.0, 'pp_iric_lstm_h64': 4.9e-08, 'tj_easy_h128': 1.06e-07}


def _build(case, switch, **over):
    import bench
    bench.WORKLOADS.setdefault('tj_easy_window', ("traffic_junction", dict(
        nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=128, ic3net=True, recurrent=True, detach_gap=4, difficulty='easy',
        add_rate_min=0.3, add_rate_max=0.3)))
    wl, flags = CASES[case]
    tr, a = bench.build_trainer(wl, E_ENVS, 5, 0, 0, **dict(flags, **over))
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=2 * E_ENVS * a.max_steps)
    a.window_launch = switch
    return tr, a


def _per_step_count(net):
    from ic3net_amd.comm import CommNetMLP
    if isinstance(net, CommNetMLP):
        return getattr(net, 'mega_steps', 0)
    return getattr(net._stand_in.get(), 'mega_steps', 0)          # models.RNN: its kernel stand-in runs the launches


def _copy(x):
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, dict):
        return {k: _copy(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_copy(v) for v in x]
    return x


def _equal(x, y, path=""):
    if torch.is_tensor(x):
        assert torch.is_tensor(y) and x.shape == y.shape and x.dtype == y.dtype, path
        if x.is_floating_point():                                  # bits (NaN-safe)
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), "%s: %d entries differ" % (path, int((x != y).sum()))
    elif isinstance(x, dict):
        assert isinstance(y, dict) and sorted(x) == sorted(y), path
        for k in x:
            _equal(x[k], y[k], "%s.%s" % (path, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), path
        for i, (u, v) in enumerate(zip(x, y)):
            _equal(u, v, "%s[%d]" % (path, i))
    elif isinstance(x, np.ndarray):
        np.testing.assert_array_equal(x, y, err_msg=path)
    else:
        assert x == y or (x != x and y != y), (path, x, y)


def _update(case, switch, before=None, **over):
    """One train_batch; returns what it rolled out (batch, records), its stat and every gradient."""
    tr, a = _build(case, switch, **over)
    if before is not None:
        before(tr, a)
    cap = {}
    inner = tr.compute_grad_native

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        cap['records'] = [dict(n=r.n, gates_n=r.gates_n, out_n=r.out_n, hs=_copy(r.hs), cs=_copy(r.cs), gates=_copy(r.gates),
                               inp=_copy(r.xh[..., :r.hs.shape[2]]), out=_copy(r.out), snaps=_copy(r.snaps), alive=_copy(r.alive), gate=_copy(r.gate),
                               h_last=_copy(r.h_last), h_last_is_slot=r.h_last_is_slot(r.n)) for r in records]
        return inner(batch, records)                               # (xh: its inp half — the backward fills in the h half)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=getattr(net, 'window_launches', 0), steps=_per_step_count(net), trainer=tr)
    return cap


def _rel_diff(g0, g1):
    assert sorted(g0) == sorted(g1)
    return {k: float((g0[k] - g1[k]).abs().max()) / max(float(g1[k].abs().max()), 1e-30) for k in g0}


@pytest.mark.parametrize("case", sorted(CASES))
def test_window_launch_update_equals_the_per_step_update(case):
    off, off2, on = _update(case, False), _update(case, False), _update(case, True)
    nwin = len(off['records'])
    assert nwin >= 2 and off['windows'] == 0 and off['steps'] == nwin * T_STEPS
    assert on['windows'] == nwin and on['steps'] == 0, "the window launch did not play every window"
    assert all(r['n'] == r['gates_n'] == r['out_n'] == T_STEPS and r['h_last_is_slot'] for r in on['records'])
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    noise, diff = _rel_diff(off2['grads'], off['grads']), _rel_diff(on['grads'], off['grads'])
    path = os.environ.get("IC3_WINDOW_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write("%-18s %d windows; largest relative gradient difference: two switch-off updates %.3e (%s), switch on vs off %.3e (%s)\n"
                    % (case, nwin, max(noise.values()), max(noise, key=noise.get), max(diff.values()), max(diff, key=diff.get)))
    # The bar is 4 x this run's own switch-off pair.  The recorded figure is a FLOOR under it, for one reason: the noise is the order
    # of a few float atomics, an ulp or two of the largest entry, and a run's pair can happen to be 0 where the switch-on update
    # then differs from it by one ulp — equality would be asked of sums that do not repeat.  Where the recorded figure is 0 too
    # (no float atomics meet in that case) the bar is 0 and equality is asserted.
    bar = 4 * max(max(noise.values()), NOISE_MEASURED[case])
    for k in diff:
        if bar == 0.0:
            assert torch.equal(on['grads'][k], off['grads'][k]), k
        else:
            assert diff[k] <= bar, (k, diff[k], bar)


def test_a_reference_gradient_fixture_passes_with_the_switch_set(monkeypatch):
    """tests/test_trainer_gpu.py's gradient fixture test, its own loading and its own bar, on arguments that carry the switch.  (The
    fixture replays the reference's action tape through a select_action of its own, so its rollout is the launch chain: the switch
    must leave that path alone.)"""
    import test_trainer_gpu as base
    build = base.build_args

    def with_switch(*args, **kw):
        a = build(*args, **kw)
        a.window_launch = True
        return a
    monkeypatch.setattr(base, 'build_args', with_switch)
    from ic3net_amd import trainer as trmod
    from ic3net_amd.comm import CommNetMLP
    seen = dict(asked=0, trainers=[], windows=0)
    ask, init, play = trmod.Trainer._window_launch_ok, trmod.Trainer.__init__, CommNetMLP.step_env_window

    def asked(self, *args, **kw):
        seen['asked'] += 1
        return ask(self, *args, **kw)

    def created(self, *args, **kw):
        seen['trainers'].append(self)
        return init(self, *args, **kw)

    def played(self, *args, **kw):
        seen['windows'] += 1
        return play(self, *args, **kw)
    monkeypatch.setattr(trmod.Trainer, '_window_launch_ok', asked)
    monkeypatch.setattr(trmod.Trainer, '__init__', created)
    monkeypatch.setattr(CommNetMLP, 'step_env_window', played)
    base.test_compute_grad_matches_reference("grad_pp_easy_ic3net", "predator_prey", True)
    # the switch was set and looked at for every episode, and left the taped rollout alone: no window was played
    assert len(seen['trainers']) == 1 and seen['trainers'][0].args.window_launch is True and seen['asked'] >= 1
    assert seen['windows'] == 0 and getattr(seen['trainers'][0].policy_net, 'window_launches', 0) == 0


@pytest.mark.parametrize("what", ["store_states", "auto_reset", "hid256", "refused"])
def test_fallbacks_run_the_per_step_path(what):
    case = 'pp_ic3net_h64'
    over = dict(hid_size=256) if what == "hid256" else {}

    def before(tr, a):
        if what == "store_states":
            a.store_states = True
        if what == "auto_reset":
            a.auto_reset = True
        if what == "refused":                                      # -38 from the library at the first window

            def refuse(*args, **kw):
                raise NotImplementedError("ic3_policy_step (ic3_policy_window): refused")
            tr.policy_net.step_env_window = refuse
    on = _update(case, True, before, **over)
    assert on['windows'] == 0 and on['steps'] > 0 and on['steps'] % T_STEPS == 0
    assert all(bool(torch.isfinite(g).all()) for g in on['grads'].values())
    if what == "refused":
        assert on['trainer']._window_refused
        off = _update(case, False)
        _equal(on['batch'], off['batch'], "batch")
        _equal(on['records'], off['records'], "records")
        _equal(on['stat'], off['stat'], "stat")

"""GPU: args.window_launch for the families of ic3_commnet_step — the non-recurrent CommNet module, the IC baseline (models.MLP),
IRIC with the tanh recurrence (models.RNN, rnn_type 'MLP'): Trainer.get_episode plays the recorded rollout of a native update as ONE
launch per window (Trainer._play_window -> step_env_commnet_window -> ic3_policy_step on an ic3_commnet_window) — against the
per-step path of the same tree: one train_batch from one seed with the switch off, again with it off, then with it on.  The batch,
the episode records (log-prob rows, snapshots, masks, counters, the h_fin record of IC, the h record of the tanh recurrence) and the
statistics must be equal bit for bit; the window counter is the number of windows and the per-step counter (commnet_steps) is 0;
every parameter gradient matches switch-off within 4 x the larger of this run's own off / off difference and the figure recorded
from the GPU run in profiles/r21/commnet_window_launch_errors.txt (IC3_WINDOW_ERRORS=<file> appends a run's figures) — where the
recorded figure is 0, equality (CommNet, IC: no float atomics meet, measured 0 / 0).  IRIC-tanh measured 6.8e-08 and 1.0e-07 between
two switch-off updates (the encoder backward's atomics) and 2.1e-07 switch on against off, the same in both visits: with h_last in
slot T of the record the heads' gradient is one product over T x R rows instead of two (bptt: h_last_is_slot).  The fallbacks (store_states, collection mode, hid 256, a window
the library refuses) run the per-step path."""
import os

import pytest
import torch

from test_window_launch_trainer_gpu import _copy, _equal, _rel_diff

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS = 8, 12

CASES = {
    'tj_easy_commnet_h128_p2': ('tj_easy_commnet_window', dict()),
    'pp_ic_h64': ('pp_hard_ic', dict(nagents=3, dim=5, vision=1, hid_size=64, max_steps=T_STEPS)),
    'pp_iric_tanh_h64': ('pp_hard_iric_tanh', dict(nagents=3, dim=5, vision=1, hid_size=64, max_steps=T_STEPS, detach_gap=4)),
}

# largest relative gradient difference between two switch-off updates from the seed, per case, as measured on the GPU
# (profiles/r21/commnet_window_launch_errors.txt, the larger of the visits' figures).  IRIC-tanh: the encoder backward's expand stage
# adds with float atomics where two agents of an env share a window cell — their order moves affine1's sums by an ulp or two of the
# largest entry from run to run
NOISE_MEASURED = {'tj_easy_commnet_h128_p2': 0.0, 'pp_ic_h64': 0.0, 'pp_iric_tanh_h64': 1.017e-07}


def _build(case, switch, **over):
    import bench
    bench.WORKLOADS.setdefault('tj_easy_commnet_window', ("traffic_junction", dict(
        nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=128, commnet=True, recurrent=False, comm_passes=2, difficulty='easy',
        add_rate_min=0.3, add_rate_max=0.3)))
    wl, flags = CASES[case]
    tr, a = bench.build_trainer(wl, E_ENVS, 5, 0, 0, **dict(flags, **over))
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=2 * E_ENVS * a.max_steps)
    a.window_launch = switch
    return tr, a


def _kernel_module(net):
    from ic3net_amd.comm import CommNetMLP
    return net if isinstance(net, CommNetMLP) else net._stand_in.get()   # the baselines: their kernel stand-in runs the launches


def _update(case, switch, before=None, **over):
    """One train_batch; returns what it rolled out (batch, records), its stat and every gradient."""
    tr, a = _build(case, switch, **over)
    if before is not None:
        before(tr, a)
    cap = {}
    inner = tr.compute_grad_native

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        cap['records'] = [dict(n=r.n, out_n=r.out_n, h_fin_n=r.h_fin_n, out=_copy(r.out), snaps=_copy(r.snaps), alive=_copy(r.alive),
                               gate=_copy(r.gate), h_fin=_copy(r.h_fin), hs=_copy(r.hs[:r.n]) if r.hs is not None else None,
                               h_last=_copy(r.h_last)) for r in records]
        cap['h_last_is_slot'] = [r.hs is not None and r.h_last_is_slot(r.n) for r in records]
        return inner(batch, records)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=getattr(net, 'window_launches', 0), steps=getattr(_kernel_module(net), 'commnet_steps', 0), trainer=tr)
    return cap


@pytest.mark.parametrize("case", sorted(CASES))
def test_window_launch_update_equals_the_per_step_update(case):
    off, off2, on = _update(case, False), _update(case, False), _update(case, True)
    nwin = len(off['records'])
    assert nwin >= 2 and off['windows'] == 0 and off['steps'] == nwin * T_STEPS
    assert on['windows'] == nwin and on['steps'] == 0, "the window launch did not play every window"
    assert all(r['n'] == r['out_n'] == T_STEPS for r in on['records'])
    if case == 'pp_ic_h64':
        assert all(r['h_fin'] is not None and r['h_fin_n'] == T_STEPS for r in on['records'])
    if case == 'pp_iric_tanh_h64':                                 # the recurrence ran in the record itself
        assert all(on['h_last_is_slot']) and all(r['hs'] is not None for r in on['records'])
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    noise, diff = _rel_diff(off2['grads'], off['grads']), _rel_diff(on['grads'], off['grads'])
    print("%-24s %d windows; largest relative gradient difference: two switch-off updates %.3e (%s), switch on vs off %.3e (%s)"
          % (case, nwin, max(noise.values()), max(noise, key=noise.get), max(diff.values()), max(diff, key=diff.get)))
    path = os.environ.get("IC3_WINDOW_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write("%-24s %d windows; largest relative gradient difference: two switch-off updates %.3e (%s), switch on vs off %.3e (%s)\n"
                    % (case, nwin, max(noise.values()), max(noise, key=noise.get), max(diff.values()), max(diff, key=diff.get)))
    bar = 4 * max(max(noise.values()), NOISE_MEASURED[case])
    for k in diff:
        if NOISE_MEASURED[case] == 0.0:
            assert torch.equal(on['grads'][k], off['grads'][k]), (k, diff[k])
        else:
            assert diff[k] <= bar, (k, diff[k], bar)


@pytest.mark.parametrize("what", ["store_states", "auto_reset", "hid256", "refused"])
def test_fallbacks_run_the_per_step_path(what):
    case = 'pp_ic_h64'
    over = dict(hid_size=256) if what == "hid256" else {}

    def before(tr, a):
        if what == "store_states":
            a.store_states = True
        if what == "auto_reset":
            a.auto_reset = True
        if what == "refused":                                      # -38 from the library at the first window

            def refuse(*args, **kw):
                raise NotImplementedError("ic3_policy_step (ic3_commnet_window): refused")
            tr.policy_net.step_env_commnet_window = refuse
    on = _update(case, True, before, **over)
    assert on['windows'] == 0 and on['steps'] % T_STEPS == 0
    # (args.store_states: ic3_commnet_step does not keep per-step states, the loop's steps are the launch chain — no counter moves)
    assert on['steps'] > 0 or what == "store_states"
    assert all(bool(torch.isfinite(g).all()) for g in on['grads'].values())
    if what == "refused":
        assert on['trainer']._window_refused
        off = _update(case, False)
        _equal(on['batch'], off['batch'], "batch")
        _equal(on['records'], off['records'], "records")
        _equal(on['stat'], off['stat'], "stat")

"""GPU: args.window_launch for recurrent CommNet / IC3Net with comm_passes 2..4 — Trainer.get_episode plays the recorded rollout of a
native update as ONE launch per window (Trainer._play_window -> CommNetMLP.step_env_window -> ic3_policy_step on an ic3_policy_window
tagged IC3_POLICY_WINDOW_PASSES) — against the per-step path of the same tree: one train_batch from one seed with the switch off, off
again, and on.  The batch, the episode records ((h, c) entering every step, log-prob rows, snapshots, masks, counters, h_last) and the
statistics must be equal bit for bit; the window counter moves and the per-step counter does not; both backwards read the record
(args.multipass_window_backward 1: the window backward, 0: the per-step loop — the path counters say which ran).

Gradients: the backward is unchanged and reads bit-equal records, so any difference is the order of the encoder's float atomics.  The
bar is 4 x the larger of the run's own switch-off pair and the largest switch-off pair seen on the GPU (NOISE_MEASURED, from
profiles/r22/multipass_window_launch_errors.txt — measured on the switch-off path, never on the window path); where both are 0,
equality.  IC3_WINDOW_ERRORS=<file> appends a run's figures.  The fallbacks (comm_passes 5, a padded twin, collection mode, a window
the library refuses) run the per-step path unchanged."""
import os

import pytest
import torch

from test_window_launch_trainer_gpu import _copy, _equal, _rel_diff

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS = 8, 12

CASES = {
    'pp_easy_p2_h64': ('pp_easy', dict(nagents=3, dim=5, vision=0, hid_size=64, max_steps=T_STEPS, detach_gap=4, comm_passes=2)),
    'tj_easy_p3_shared_h128': ('tj_easy_window', dict(comm_passes=3, share_weights=True)),
}

# largest relative gradient difference between two switch-off updates from the seed, per (case, multipass_window_backward), as measured
# on the GPU (profiles/r22/multipass_window_launch_errors.txt; the encoder's expand stage adds with float atomics, whose order moves
# the sums by an ulp or two of the largest entry from run to run — 0 where no two agents of an env share a window cell)
NOISE_MEASURED = {('pp_easy_p2_h64', 1): 0.0, ('pp_easy_p2_h64', 0): 2.76e-07,
                  ('tj_easy_p3_shared_h128', 1): 9.16e-08, ('tj_easy_p3_shared_h128', 0): 3.12e-07}


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


def _update(case, switch, before=None, **over):
    """One train_batch; returns what it rolled out (batch, records), its stat, every gradient and the path counters."""
    tr, a = _build(case, switch, **over)
    if before is not None:
        before(tr, a)
    cap = {}
    inner = tr.compute_grad_native

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        # (slot n of (hs, cs) belongs to nobody behind a per-step rollout of this family: h_last holds the final state)
        cap['records'] = [dict(n=r.n, gates_n=r.gates_n, out_n=r.out_n, has_gates=r.gates is not None, hs=_copy(r.hs[:r.n]),
                               cs=_copy(r.cs[:r.n]), out=_copy(r.out), snaps=_copy(r.snaps), alive=_copy(r.alive), gate=_copy(r.gate),
                               h_last=_copy(r.h_last), h_last_is_slot=r.h_last_is_slot(r.n)) for r in records]
        return inner(batch, records)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    km = net.kernel_module()                                       # (hid 48: the zero-padded twin runs the launches)
    count = lambda name: getattr(net, name, 0) + (getattr(km, name, 0) if km is not net else 0)
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=count('window_launches'), steps=count('mega_steps'), trainer=tr,
               window_backwards=getattr(net, 'multipass_window_backwards', 0), loop_backwards=getattr(net, 'multipass_loop_backwards', 0))
    return cap


@pytest.mark.parametrize("window_backward", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_window_launch_update_equals_the_per_step_update(case, window_backward):
    over = dict(multipass_window_backward=bool(window_backward))
    off, off2, on = _update(case, False, **over), _update(case, False, **over), _update(case, True, **over)
    nwin = len(off['records'])
    assert nwin >= 2 and off['windows'] == 0 and off['steps'] == nwin * T_STEPS
    assert on['windows'] == nwin and on['steps'] == 0, "the window launch did not play every window"
    assert all(r['n'] == r['out_n'] == T_STEPS and r['gates_n'] == 0 and not r['has_gates'] for r in on['records'])
    for run in (off, on):                                          # which backward read the record
        assert (run['window_backwards'], run['loop_backwards']) == ((nwin, 0) if window_backward else (0, nwin)), \
            (run['window_backwards'], run['loop_backwards'])
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    noise, diff = _rel_diff(off2['grads'], off['grads']), _rel_diff(on['grads'], off['grads'])
    path = os.environ.get("IC3_WINDOW_ERRORS")
    line = ("%-24s window_backward %d: %d windows; largest relative gradient difference: two switch-off updates %.3e (%s), "
            "switch on vs off %.3e (%s)" % (case, window_backward, nwin, max(noise.values()), max(noise, key=noise.get),
                                            max(diff.values()), max(diff, key=diff.get)))
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    # 4 x the larger of this run's own switch-off pair and the recorded one (a run's pair can happen to be 0 where the sums do not
    # repeat); both 0: no float atomics meet in that case, and equality is asserted
    bar = 4 * max(max(noise.values()), NOISE_MEASURED[(case, window_backward)])
    for k in diff:
        if bar == 0.0:
            assert torch.equal(on['grads'][k], off['grads'][k]), k
        else:
            assert diff[k] <= bar, (k, diff[k], bar)


@pytest.mark.parametrize("what", ["passes5", "hid48", "auto_reset", "refused"])
def test_fallbacks_run_the_per_step_path(what):
    case = 'pp_easy_p2_h64'
    over = dict(comm_passes=5) if what == "passes5" else dict(hid_size=48) if what == "hid48" else {}

    def before(tr, a):
        if what == "auto_reset":
            a.auto_reset = True
        if what == "refused":                                      # -38 from the library at the first window

            def refuse(*args, **kw):
                raise NotImplementedError("ic3_policy_step (ic3_policy_window, passes): refused")
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

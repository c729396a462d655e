"""GPU: args.window_launch_collection — Trainer._run_batch_streams (collection mode, args.auto_reset) plays every window of a recorded
native update as ONE launch (Trainer._play_window): the window that starts the E streams and the two that continue them, step 0 handed
the previous window's masks and state, the restarts inside the launch — against the per-step path of the same tree.

One train_batch from one seed with auto_reset and window_launch set and the new flag 0, a second one with flag 0, one with flag 1.  The
batch, the episode records (the state record, gates, inp rows, log-prob rows, snapshots, masks, the cuts of the streams, the counters)
and the statistics must be equal bit for bit; with flag 1 the window counter counts every window and the per-step counter stays 0, with
flag 0 the reverse; every parameter gradient matches flag 0 within 4 x the largest relative difference between the TWO flag-0 updates
(measured in the run itself, with the figure recorded in profiles/r23/collection_window_errors.txt as a floor under it;
IC3_WINDOW_ERRORS=<file> appends a run's figures) — where that is 0 in every recorded run, equality.  The fallbacks (store_states, hid
256, comm_passes 5, a window the library refuses) run the per-step path unchanged."""
import os

import pytest
import torch

from test_window_launch_trainer_gpu import _copy, _equal, _rel_diff

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS, WINDOWS = 8, 12, 3

# (workload, flags, the per-step counter's family).  PP IC3Net: a 2 x 2 grid, so that predators meet the prey — and episodes end — well
# before max_steps: the streams of those envs leave the window boundaries (asserted below)
CASES = {
    'pp_ic3net_h64': ('pp_easy', dict(nagents=3, dim=2, vision=0, hid_size=64, max_steps=T_STEPS, detach_gap=4), 'mega'),
    'tj_easy_h128': ('tj_easy_window', dict(), 'mega'),
    'pp_iric_lstm_h64': ('pp_hard_iric', dict(nagents=3, dim=5, vision=1, hid_size=64, max_steps=T_STEPS, detach_gap=4), 'mega'),
    'pp_p2_h64_loop': ('pp_easy', dict(nagents=3, dim=2, vision=0, hid_size=64, max_steps=T_STEPS, detach_gap=4, comm_passes=2,
                                      multipass_window_collection=0), 'mega'),
    'pp_p2_h64_window': ('pp_easy', dict(nagents=3, dim=2, vision=0, hid_size=64, max_steps=T_STEPS, detach_gap=4, comm_passes=2,
                                        multipass_window_collection=1), 'mega'),
    'pp_ic_h64': ('pp_hard_ic', dict(nagents=3, dim=5, vision=1, hid_size=64, max_steps=T_STEPS), 'commnet'),
    'pp_iric_tanh_h64': ('pp_hard_iric_tanh', dict(nagents=3, dim=5, vision=1, hid_size=64, max_steps=T_STEPS, detach_gap=4), 'commnet'),
    'tj_easy_commnet_h128_p2': ('tj_easy_commnet_window', dict(), 'commnet'),
}

# largest relative gradient difference between two flag-0 updates from the seed, per case, as measured on the GPU
# (profiles/r23/collection_window_errors.txt; the encoder backward's expand stage adds with float atomics where two agents of an env
# share a window cell — their order moves the sums by an ulp or two of the largest entry from run to run)
NOISE_MEASURED = {'pp_ic3net_h64': 0.0, 'tj_easy_h128': 9.747e-08, 'pp_iric_lstm_h64': 5.170e-08, 'pp_p2_h64_loop': 8.617e-08,
                  'pp_p2_h64_window': 0.0, 'pp_ic_h64': 0.0, 'pp_iric_tanh_h64': 1.401e-07, 'tj_easy_commnet_h128_p2': 0.0}


def _build(case, flag, **over):
    import bench
    bench.WORKLOADS.setdefault('tj_easy_window', ("traffic_junction", dict(
        nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=128, ic3net=True, recurrent=True, detach_gap=4, difficulty='easy',
        add_rate_min=0.3, add_rate_max=0.3)))
    bench.WORKLOADS.setdefault('tj_easy_commnet_window', ("traffic_junction", dict(
        nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=128, commnet=True, recurrent=False, comm_passes=2, difficulty='easy',
        add_rate_min=0.3, add_rate_max=0.3)))
    wl, flags, _ = CASES[case]
    tr, a = bench.build_trainer(wl, E_ENVS, 5, 0, 0, **dict(flags, **over))
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=WINDOWS * E_ENVS * a.max_steps)
    a.auto_reset = True
    a.window_launch = True
    a.window_launch_collection = flag
    return tr, a


def _count(net, name):
    """A per-step path counter, read where the existing window tests read it: on the policy itself, or — the baselines — on the
    kernel stand-in that runs their launches."""
    from ic3net_amd.comm import CommNetMLP
    return getattr(net if isinstance(net, CommNetMLP) else net._stand_in.get(), name, 0)


def _record(r, lstm):
    n, H = r.n, r.hs.shape[2] if r.hs is not None else 0
    d = dict(n=r.n, gates_n=r.gates_n, out_n=r.out_n, h_fin_n=r.h_fin_n, out=_copy(r.out), snaps=_copy(r.snaps), alive=_copy(r.alive),
             gate=_copy(r.gate), h_last=_copy(r.h_last), h_fin=_copy(r.h_fin), stream=_copy(r.stream), has_gates=r.gates is not None)
    if r.hs is not None:                                           # (slot n: h_last holds what the window ended with)
        d['hs'] = _copy(r.hs[:n])
    if lstm:
        d['cs'] = _copy(r.cs[:n])
    if r.gates is not None:                                        # (xh: its inp half — the backward fills in the h half)
        d.update(gates=_copy(r.gates), inp=_copy(r.xh[..., :H]))
    return d


def _update(case, flag, before=None, **over):
    """One train_batch in collection mode; returns what it rolled out (batch, records), its stat, every gradient and the counters."""
    tr, a = _build(case, flag, **over)
    if before is not None:
        before(tr, a)
    cap = {}
    inner = tr.compute_grad_native
    lstm = bool(a.recurrent) and a.rnn_type == 'LSTM'

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        cap['records'] = [_record(r, lstm) for r in records]
        return inner(batch, records)
    tr.compute_grad_native = spy
    stat = tr.train_batch(0)
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    # (a baseline counts a window on itself and on its stand-in: the policy's own counter is the number of windows)
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=getattr(net, 'window_launches', 0), trainer=tr,
               steps=_count(net, 'mega_steps' if CASES[case][2] == 'mega' else 'commnet_steps'))
    return cap


_RUNS = {}


def _runs(case):
    """(flag 0, flag 0 again, flag 1) of a case, played once."""
    if case not in _RUNS:
        _RUNS[case] = (_update(case, 0), _update(case, 0), _update(case, 1))
    return _RUNS[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_collection_window_update_equals_the_per_step_update(case):
    off, off2, on = _runs(case)
    assert len(off['records']) == len(on['records']) == WINDOWS
    assert off['windows'] == 0 and off['steps'] == WINDOWS * T_STEPS
    assert on['windows'] == WINDOWS and on['steps'] == 0, "the window launch did not play every collection window"
    assert all(r['n'] == r['out_n'] == T_STEPS and r['stream'] is not None for r in on['records'])
    assert [(r['stream']['first'], r['stream']['last']) for r in on['records']] == [(True, False), (False, False), (False, True)]
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    done = torch.stack([m['done'] for m in off['batch'][8]]).reshape(WINDOWS, T_STEPS, E_ENVS)
    early = int(done[:, :T_STEPS - 1].any(1).any(0).sum())
    noise, diff = _rel_diff(off2['grads'], off['grads']), _rel_diff(on['grads'], off['grads'])
    line = ("%-24s %d windows, %d of %d envs end an episode before a window's last slot; largest relative gradient difference: two "
            "flag-0 updates %.3e (%s), flag 1 vs flag 0 %.3e (%s)" % (case, WINDOWS, early, E_ENVS, max(noise.values()),
                                                                      max(noise, key=noise.get), max(diff.values()), max(diff, key=diff.get)))
    print(line)
    path = os.environ.get("IC3_WINDOW_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    if case == 'pp_ic3net_h64':                                    # what takes the streams off the window boundaries
        assert early >= 2, "%d envs end an episode before a window's last slot" % early
    # 4 x the larger of this run's own flag-0 pair and the recorded one (a run's pair can happen to be 0 where the sums do not
    # repeat); both 0: no float atomics meet in that case, and equality is asserted
    bar = 4 * max(max(noise.values()), NOISE_MEASURED[case])
    for k in diff:
        if bar == 0.0:
            assert torch.equal(on['grads'][k], off['grads'][k]), (k, diff[k])
        else:
            assert diff[k] <= bar, (k, diff[k], bar)


@pytest.mark.parametrize("what", ["store_states", "hid256", "passes5", "refused"])
def test_fallbacks_run_the_per_step_path(what):
    case = 'pp_ic3net_h64'
    over = dict(hid_size=256) if what == "hid256" else dict(comm_passes=5) if what == "passes5" else {}

    def before(tr, a):
        if what == "store_states":
            a.store_states = True
        if what == "refused":                                      # -38 from the library at the first window

            def refuse(*args, **kw):
                raise NotImplementedError("ic3_policy_step (ic3_policy_window): refused")
            tr.policy_net.step_env_window = refuse
    on = _update(case, 1, before, **over)
    assert on['windows'] == 0 and on['steps'] == WINDOWS * T_STEPS
    assert all(bool(torch.isfinite(g).all()) for g in on['grads'].values())
    if what == "refused":
        assert on['trainer']._window_refused
        off = _runs(case)[0]
        _equal(on['batch'], off['batch'], "batch")
        _equal(on['records'], off['records'], "records")
        _equal(on['stat'], off['stat'], "stat")

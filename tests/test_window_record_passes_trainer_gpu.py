"""GPU: args.window_record_passes — the window launch of a comm_passes 2..4 policy (args.window_launch) also records what its passes
computed (ic3_policy_step on an ic3_policy_window_record), and bptt._backward_window_multipass reads that record instead of
re-evaluating the passes.  One train_batch from one seed with the flag off and on, at the shapes of
tests/test_multipass_window_launch_trainer_gpu.py (lock-step PP with two passes, TJ with three shared passes) and one
collection-mode pair of windows:

  flag on    every window is counted in multipass_recorded_windows; the update makes no ops.policy_forward_record call and no
             encode_at call inside the backward (counting wrappers)
  flag off   the counts are the parent's: P recording forwards and T encode_at calls per window (one chunk per window here)
  rollout    batch, statistics and the (h, c) record are bit-equal with the flag on and off
  gradients  every parameter, on against off, within tests/window_record_bars.TRAINER_BARS: 4 x the measured worst
             |on - off| / max |off|, never above 1e-5 (profiles/r28/window_record_errors.txt).  Bit equality is not asked for: the
             record holds what the rollout's cells used, the re-evaluation rounds pass i > 0's encoder bias differently
  fallbacks  with the memory room forced to zero the flag changes nothing and the re-evaluation runs; a refused window leaves no
             partial record in use."""
import json
import os

import pytest
import torch

from test_window_launch_trainer_gpu import _copy, _equal, _rel_diff

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS = 8, 12

CASES = {
    'pp_easy_p2_h64': ('pp_easy', dict(nagents=3, dim=5, vision=0, hid_size=64, max_steps=T_STEPS, detach_gap=4, comm_passes=2), {}),
    'tj_easy_p3_shared_h128': ('tj_easy_window', dict(comm_passes=3, share_weights=True), {}),
    # collection mode: two windows of E streams, episodes ending and starting inside them (tests/test_multipass_collection_window_trainer_gpu.py)
    'pp_tiny_collection_p2_h64': ('pp_easy', dict(comm_passes=2, hid_size=64, nagents=2, dim=3, vision=1, max_steps=T_STEPS, detach_gap=5),
                                  dict(auto_reset=True, window_launch_collection=1, multipass_window_collection=1, E=32, windows=2)),
}


def _build(case, record, **over):
    import bench
    bench.WORKLOADS.setdefault('tj_easy_window', ("traffic_junction", dict(
        nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=128, ic3net=True, recurrent=True, detach_gap=4, difficulty='easy',
        add_rate_min=0.3, add_rate_max=0.3)))
    wl, flags, mode = CASES[case]
    E, nwin = mode.get('E', E_ENVS), mode.get('windows', 2)
    tr, a = bench.build_trainer(wl, E, 5, 0, 0, **dict(flags, **over))
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=nwin * E * a.max_steps)
    a.__dict__.update({k: v for k, v in mode.items() if k not in ('E', 'windows')})
    a.window_launch = True
    a.window_record_passes = int(record)
    return tr, a


def _update(case, record, before=None, **over):
    """One train_batch; returns what it rolled out, its stat, every gradient, the path counters and the counted calls."""
    from ic3net_amd import ops
    tr, a = _build(case, record, **over)
    if before is not None:
        before(tr, a)
    cap = dict(forward_record=0, encode_at=0)
    inner, raw = tr.compute_grad_native, tr.env.env
    real_forward, real_encode = ops.policy_forward_record, raw.encode_at
    state = dict(backward=False)

    def forward_record(*args, **kw):
        cap['forward_record'] += 1
        return real_forward(*args, **kw)

    def encode_at(*args, **kw):
        cap['encode_at'] += int(state['backward'])
        return real_encode(*args, **kw)

    def spy(batch, records):
        cap['batch'] = _copy(list(batch))
        cap['records'] = [dict(n=r.n, out_n=r.out_n, hs=_copy(r.hs[:r.n]), cs=_copy(r.cs[:r.n]), out=_copy(r.out), snaps=_copy(r.snaps),
                               alive=_copy(r.alive), gate=_copy(r.gate), h_last=_copy(r.h_last)) for r in records]
        cap['pass_n'] = [r.pass_n for r in records]
        cap['has_record'] = [r.pass_gates is not None for r in records]
        state['backward'] = True
        try:
            return inner(batch, records)
        finally:
            state['backward'] = False
    tr.compute_grad_native = spy
    ops.policy_forward_record, raw.encode_at = forward_record, encode_at
    try:
        stat = tr.train_batch(0)
    finally:
        ops.policy_forward_record = real_forward
        del raw.encode_at
    torch.cuda.synchronize()
    assert 'batch' in cap, "the native update did not run"
    net = tr.policy_net
    cap.update(stat=stat, grads={k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
               windows=getattr(net, 'window_launches', 0), steps=getattr(net, 'mega_steps', 0), trainer=tr, passes=net.comm_passes,
               window_backwards=getattr(net, 'multipass_window_backwards', 0), loop_backwards=getattr(net, 'multipass_loop_backwards', 0),
               recorded=getattr(net, 'multipass_recorded_windows', 0), chunk=getattr(net, 'multipass_window_chunk', None))
    return cap


def _parent_counts(run, nwin):
    """What the re-evaluating window backward calls: P recording forwards per chunk, one encode_at per step."""
    chunks = -(-T_STEPS // run['chunk'])
    return nwin * chunks * run['passes'], nwin * T_STEPS


@pytest.mark.parametrize("case", sorted(CASES))
def test_recorded_update_against_the_re_evaluating_update(case):
    from window_record_bars import TRAINER_BARS
    off, on = _update(case, 0), _update(case, 1)
    nwin = len(off['records'])
    assert nwin == 2 and len(on['records']) == nwin
    for run in (off, on):                                          # both play every window in one launch, both run the window backward
        assert run['windows'] == nwin and run['steps'] == 0 and (run['window_backwards'], run['loop_backwards']) == (nwin, 0), run
    # flag on: every window recorded and read; no recording forward, no encoder ring
    assert on['has_record'] == [True] * nwin and on['pass_n'] == [T_STEPS] * nwin
    assert on['recorded'] == nwin and on['forward_record'] == 0 and on['encode_at'] == 0, (on['recorded'], on['forward_record'], on['encode_at'])
    # flag off: the parent's counts
    assert off['has_record'] == [False] * nwin and off['recorded'] == 0
    assert (off['forward_record'], off['encode_at']) == _parent_counts(off, nwin), (off['forward_record'], off['encode_at'])
    # the rollout is the same rollout
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")
    diff = _rel_diff(on['grads'], off['grads'])
    for k in sorted(diff):
        print("window-record gpu/trainer-%s %s %.3e" % (case, k, diff[k]))
    path = os.environ.get('IC3_WINDOW_RECORD_ERRORS_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case='gpu/trainer-' + case, errs=diff)) + "\n")
    assert all(bool(torch.isfinite(g).all()) for g in on['grads'].values())
    bars = TRAINER_BARS.get('gpu/trainer-' + case, {})
    bad = {k: (v, bars.get(k)) for k, v in diff.items() if not (k in bars and v <= bars[k])}
    assert not bad, "%s: (measured, bar) %r" % (case, bad)


def test_no_memory_room_means_no_record_and_the_re_evaluation():
    from ic3net_amd import bptt
    case = 'pp_easy_p2_h64'

    def before(tr, a):                                             # no room while the episode's buffers are allocated — there only
        begin = tr.begin_episode

        def begin_episode(epoch):
            real = bptt.device_room
            bptt.device_room = lambda dev: 0
            try:
                return begin(epoch)
            finally:
                bptt.device_room = real
        tr.begin_episode = begin_episode
    off, on = _update(case, 0), _update(case, 1, before)
    nwin = len(off['records'])
    assert on['has_record'] == [False] * nwin and on['recorded'] == 0 and on['windows'] == nwin
    assert (on['forward_record'], on['encode_at']) == (off['forward_record'], off['encode_at']) == _parent_counts(off, nwin)
    _equal(on['batch'], off['batch'], "batch")
    _equal(on['records'], off['records'], "records")
    _equal(on['stat'], off['stat'], "stat")


def test_a_refused_window_leaves_no_partial_record_in_use():
    case = 'pp_easy_p2_h64'

    def before(tr, a):                                             # -38 from the library at the first window

        def refuse(*args, **kw):
            raise NotImplementedError("ic3_policy_step (ic3_policy_window, passes record): refused")
        tr.policy_net.step_env_window = refuse
    on = _update(case, 1, before)
    nwin = len(on['records'])
    assert on['trainer']._window_refused and on['windows'] == 0 and on['steps'] == nwin * T_STEPS
    assert on['pass_n'] == [0] * nwin and on['recorded'] == 0, "a record nobody completed was read"
    assert on['window_backwards'] == nwin and (on['forward_record'], on['encode_at']) == _parent_counts(on, nwin)
    assert all(bool(torch.isfinite(g).all()) for g in on['grads'].values())

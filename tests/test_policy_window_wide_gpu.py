"""GPU: `ic3_policy_step` on an `ic3_policy_window` tagged IC3_POLICY_WINDOW_WIDE — T lock-steps of the recorded training rollout at
hid 256 in ONE launch (policy_step_kernel<256, KIND, 1, 0, 0, 1>: one workgroup of 512 threads per CU) — against T per-step launches
of the same library on a twin handle, BIT FOR BIT: the (h, c) record, the gate record, the inp record (the inp rows alone, row stride
H: what ic3_env_set_record_out writes per step at this width), out, action, reward, done, alive, is_completed, all T snapshots and the
state the handle is left in.

The cases are those of tests/test_host_window_wide_cpu.py, plus what only the device has: more tiles than workgroup slots (one per CU
at this width: a CU plays a second tile with its vector L1 warm with the lines of the first — the hand-off between two steps of a
workgroup must not read them), the window twice from the same state, the window on the caller's non-default stream, and the answers
of the *_supported queries."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_policy_window_gpu import _same, _setup  # noqa: E402

H = 256
CASES = {
    # 21 envs per 64-row tile: one full and one ragged tile; the gate chain
    'pp': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=H, hard_attn=True, E=23, T=3),
    # the alive slice of step t - 1 is step t's mask; a gate of ones
    'tj_easy': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=H,
                    hard_attn=False, ones=True, E=14, T=4),
    # auto-reset: episodes of 2 steps restart inside the window
    'pp_auto': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=H, hard_attn=True, auto=2, E=23, T=5),
}


def _buffers(env, heads, E, n):
    from ic3net_amd import ops
    N, dev = env.nagents_env, env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    assert ops.record_xh_width(H) == H
    b = dict(hs=f(n + 1, R, H), cs=f(n + 1, R, H), gates=f(n, R, 4 * H), inp=f(n, R, H), out=f(n, R, OT), action=i(n, nh, E, N),
             reward=f(n, E, N), done=i(n, E), alive=i(n, E, N), comp=i(n, E, N), snaps=i(n, env.dims.state_words))
    g = torch.Generator(device='cpu').manual_seed(11)
    b['hs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    b['cs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    return b


def _play(w, windows, E=None):
    """windows = 0: nwin * T per-step launches; otherwise that many consecutive window launches of T steps, each continuing the one
    before (its masks, its slot T as slot 0).  One record of all slots either way."""
    from ic3net_amd import ops
    E, T = E or w['E'], w['T']
    env, net, fc, heads = _setup(w, E)
    N, dev = env.nagents_env, env.device
    nh = len(heads)
    nwin = max(windows, 1) if windows else w.get('nwin', 1)
    n = nwin * T
    b = _buffers(env, heads, E, n)
    tj = w['kind'] == 'tj'
    ones = torch.ones((E, N), dtype=torch.int32, device=dev) if w.get('ones') else None
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else ones
    after = lambda t: (b['alive'][t] if tj else None, b['action'][t, nh - 1] if w['hard_attn'] else ones)
    with torch.no_grad():
        if windows:
            assert ops.policy_step_window_supported(env, fc, H, wide=True)
            for k in range(nwin):
                s = slice(k * T, (k + 1) * T)
                # (a window's (h, c) record is T + 1 contiguous slots: slots kT .. kT + T of the joint record)
                ops.policy_step_window(env, fc, H, heads, True, False, T, b['hs'][k * T:(k + 1) * T + 1], b['cs'][k * T:(k + 1) * T + 1],
                                       alive_in, comm_in, b['out'][s], b['action'][s], b['reward'][s], b['done'][s], b['alive'][s],
                                       b['comp'][s], gates=b['gates'][s], inp=b['inp'][s], snaps=b['snaps'][s], alive_prev=tj,
                                       comm_mode='last_head' if w['hard_attn'] else 'ones' if w.get('ones') else 'all', wide=True)
                alive_in, comm_in = after((k + 1) * T - 1)
        else:
            for t in range(n):
                env.snapshot(out=b['snaps'][t])
                env.set_hidden_out(b['hs'][t + 1], b['cs'][t + 1])
                env.set_record_out(b['gates'][t], b['inp'][t])
                ops.policy_step(env, fc, H, heads, True, False, b['hs'][t], b['cs'][t], alive_in, comm_in, b['out'][t], b['action'][t],
                                b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t])
                alive_in, comm_in = after(t)
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['t_field'] = env.get_state()['t']
    return b


_REF = {}


def _ref(name, nwin=1):
    key = (name, nwin)
    if key not in _REF:
        _REF[key] = _play(dict(CASES[name], nwin=nwin), 0)
    return _REF[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_wide_window_launch_writes_the_bits_of_T_per_step_launches(name):
    w = CASES[name]
    ref, win = _ref(name), _play(w, 1)
    _same(win, ref, name)
    T = w['T']
    assert bool(torch.isfinite(ref['hs']).all()) and bool(torch.isfinite(ref['out']).all()) and bool((ref['action'] >= 0).all())
    assert bool(torch.isfinite(ref['gates']).all()) and bool(torch.isfinite(ref['inp']).all())
    if name == 'pp':
        gate = ref['action'][:, -1]
        assert bool((gate == 0).any()) and bool((gate == 1).any()), "the gate chain carries one value only"
    if name == 'tj_easy':
        assert bool((ref['alive'][1:] != ref['alive'][:-1]).any()), "no car's alive flag changes inside the window"
    if name == 'pp_auto':
        assert bool(ref['done'][:T - 1].any()), "no episode ends inside the window"


def test_two_consecutive_wide_windows_write_the_bits_of_2T_per_step_launches():
    w = CASES['pp_auto']
    T = w['T']
    ref, win = _ref('pp_auto', 2), _play(w, 2)
    _same(win, ref, "two windows")
    done = ref['done'].to(torch.bool)
    assert bool(done[:T - 1].any()) and bool(done[T:2 * T - 1].any()), "no episode ends inside one of the windows"


def _many_tiles():
    """More tiles than workgroup slots (ONE workgroup per CU at hid 256) + 64: N 10 -> 6 envs per tile."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    E = 6 * (cus + 64) + 3
    w = dict(kind='pp', env=dict(N=10, dim=5, vision=0, mode='mixed'), H=H, hard_attn=True, E=E, T=4)
    if 'many' not in _REF:
        _REF['many'] = (_play(w, 0), _play(w, 1), w)
    return _REF['many']


def test_more_tiles_than_workgroup_slots():
    ref, win, w = _many_tiles()
    _same(win, ref, "E = %d" % w['E'])


def test_the_window_twice_from_the_same_state_is_the_same_bits():
    _, win, w = _many_tiles()
    _same(_play(w, 1), win, "second play, E = %d" % w['E'])


def test_the_window_on_the_callers_stream():
    w = CASES['tj_easy']
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        win = _play(w, 1)
    side.synchronize()
    _same(win, _ref('tj_easy'), "side stream")


def test_supported_answers_and_refusals():
    from ic3net_amd import ops
    from ic3net_amd.comm import CommNetMLP
    for hid in (64, 128, 256):
        env, net, fc, heads = _setup(dict(CASES['pp'], H=hid), 5)
        assert ops.policy_step_window_supported(env, fc, hid, wide=True) == (hid == 256)
        assert ops.policy_step_window_supported(env, fc, hid) == (hid != 256)          # the narrow tag's answers stay
        assert not ops.policy_step_window_supported(env, fc, hid, passes=2, wide=True)
        with torch.no_grad():                                      # (the grad mode a recorded rollout runs in)
            assert net.window_supported(env, wide=True) and net.window_supported(env) == (hid != 256)
    # hid 256 stays in `env, fc, heads`.  A descriptor of the narrow tag is still refused there, the wide one at another width too
    N, T, R = 3, 2, 15
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    args = lambda hid: (hid, heads, True, False, T, z(T + 1, R, hid), z(T + 1, R, hid), None, None, z(T, R, 8),
                        z(T, 2, 5, N, dt=torch.int32), z(T, 5, N), z(T, 5, dt=torch.int32))
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window\)"):
        ops.policy_step_window(env, fc, *args(256))
    with pytest.raises(AssertionError):
        ops.policy_step_window(env, fc, *args(64), wide=True)
    env.set_hidden_out(z(R, H), z(R, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_policy_window, wide\)"):
        ops.policy_step_window(env, fc, *args(256), wide=True)
    ops.policy_step_window(env, fc, *args(256), wide=True)         # disarmed by the refused call
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window, wide\)"):
        ops.policy_step_window(env, dict(fc, ps_l_wp3=None), *args(256), wide=True)
    # a zero-padded twin (hid 200 runs the kernels at 256 with wider rows than the record's) keeps answering no
    env.reset()
    torch.manual_seed(3)
    twin = CommNetMLP(argparse.Namespace(nagents=N, hid_size=200, comm_passes=1, recurrent=True, continuous=False, naction_heads=heads,
                                         comm_mask_zero=False, share_weights=False, comm_init='uniform', hard_attn=True,
                                         comm_mode='avg', rnn_type='LSTM', init_std=0.2), env.obs_dim).cuda().float()
    twin.obs_encoder, twin.obs_table = env.encode, env.encode_table
    with torch.no_grad():
        assert ops.padded_hidden(200) == 256
        assert not twin.window_supported(env, wide=True) and not twin.window_supported(env)

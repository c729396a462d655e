"""GPU: `ic3_policy_step` on an `ic3_policy_window` — T lock-steps of the recorded training rollout in ONE launch (the WIN
instantiations of csrc/policy_step.hip) — against T per-step launches of the same library on a twin handle, BIT FOR BIT: the (h, c)
record, the gate / inp records, out, action, reward, done, alive, is_completed, all T snapshots and the state the handle is left in.

The per-step side plays what the Trainer's recorded rollout plays: ic3_env_snapshot in front of the step, ic3_env_set_hidden_out to
slot t + 1, ic3_env_set_record_out to the step's rows, the masks of step t - 1 handed over.  The shapes are those of
tests/test_host_policy_window_cpu.py, plus: more tiles than the device has workgroup slots (a CU plays several tiles in turn, its
vector L1 warm with the lines of the tile before — the hand-off between two steps of a workgroup must not read them), the window
twice from the same state, and the window on the caller's non-default stream."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_env_parity_gpu import make_pp, make_tj  # noqa: E402

KEYS = ('hs', 'cs', 'gates', 'inp', 'out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps')

CASES = {
    'pp': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=64, hard_attn=True, E=45, T=6),
    'tj_easy': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=128,
                    hard_attn=True, E=26, T=8),
    'pp_auto': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=64, hard_attn=False, ones=True, auto=3, E=45, T=7),
    'pp_done': dict(kind='pp', env=dict(N=2, dim=3, vision=1, mode='mixed'), H=64, hard_attn=False, E=40, T=8),
}


def _setup(w, E, seed=7, offset=40):
    from ic3net_amd.comm import CommNetMLP
    kw = dict(w['env'])
    if w['kind'] == 'pp':
        env = make_pp(kw.pop('N'), kw.pop('dim'), kw.pop('vision'), kw.pop('mode'), E, seed=seed, offset=offset, **kw)
        env.reset()
    else:
        env = make_tj(kw.pop('N'), kw.pop('dim'), kw.pop('vision'), kw.pop('difficulty'), E, seed=seed, offset=offset, **kw)
        env.reset(0)
    if w.get('auto'):
        env.set_auto_reset(w['auto'])
    N, H = env.nagents_env, w['H']
    heads = [env.dims.naction, 2] if (w['hard_attn'] or w.get('ones')) else [env.dims.naction]
    torch.manual_seed(H + N)
    net = CommNetMLP(argparse.Namespace(nagents=N, hid_size=H, comm_passes=1, recurrent=True, continuous=False, naction_heads=heads,
                                        comm_mask_zero=False, share_weights=False, comm_init='uniform', hard_attn=w['hard_attn'],
                                        comm_mode='avg', rnn_type='LSTM', init_std=0.2), env.obs_dim).cuda().float()
    with torch.no_grad():
        for hd in net.heads:
            hd.weight.mul_(4.0)
        net.obs_encoder, net.obs_table = env.encode, env.encode_table
        fc = net._fused_cache()
    return env, net, fc, heads


def _play(w, window, E=None, T=None):
    from ic3net_amd import ops
    E, T = E or w['E'], T or w['T']
    env, net, fc, heads = _setup(w, E)
    N, H, dev = env.nagents_env, w['H'], env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(hs=f(T + 1, R, H), cs=f(T + 1, R, H), gates=f(T, R, 4 * H), inp=f(T, R, 2 * H), out=f(T, R, OT), action=i(T, nh, E, N),
             reward=f(T, E, N), done=i(T, E), alive=i(T, E, N), comp=i(T, E, N), snaps=i(T, env.dims.state_words))
    g = torch.Generator(device='cpu').manual_seed(11)
    b['hs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    b['cs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    tj = w['kind'] == 'tj'
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else \
        torch.ones((E, N), dtype=torch.int32, device=dev) if w.get('ones') else None
    with torch.no_grad():
        if window:
            assert ops.policy_step_window_supported(env, fc, H)
            ops.policy_step_window(env, fc, H, heads, True, False, T, b['hs'], b['cs'], alive_in, comm_in, b['out'], b['action'],
                                   b['reward'], b['done'], b['alive'], b['comp'], gates=b['gates'], inp=b['inp'], snaps=b['snaps'],
                                   alive_prev=tj, comm_mode='last_head' if w['hard_attn'] else 'ones' if w.get('ones') else 'all')
        else:
            for t in range(T):
                env.snapshot(out=b['snaps'][t])
                env.set_hidden_out(b['hs'][t + 1], b['cs'][t + 1])
                env.set_record_out(b['gates'][t], b['inp'][t])
                ops.policy_step(env, fc, H, heads, True, False, b['hs'][t], b['cs'][t], alive_in, comm_in, b['out'][t], b['action'][t],
                                b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t])
                if tj:
                    alive_in = b['alive'][t]
                if w['hard_attn']:
                    comm_in = b['action'][t, nh - 1]
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['t_field'] = env.get_state()['t']
    return b


def _same(a, b, what):
    for key in KEYS + ('state',):
        x, y = a[key], b[key]
        same = torch.equal(x.view(torch.int32), y.view(torch.int32))      # bits (the untouched halves of inp hold NaN on both sides)
        assert same, "%s: %s differs in %d words" % (what, key, int((x.view(torch.int32) != y.view(torch.int32)).sum()))


_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = _play(CASES[name], False)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_window_launch_writes_the_bits_of_T_per_step_launches(name):
    w = CASES[name]
    ref, win = _ref(name), _play(w, True)
    _same(win, ref, name)
    T = w['T']
    assert bool(torch.isfinite(ref['hs']).all()) and bool(torch.isfinite(ref['out']).all()) and bool((ref['action'] >= 0).all())
    if name == 'tj_easy':
        assert bool((ref['alive'][1:] != ref['alive'][:-1]).any()), "no car's alive flag changes inside the window"
    if name == 'pp_auto':
        assert bool(ref['done'][:T - 1].any()), "no episode ends inside the window"
    if name == 'pp_done':
        assert bool(ref['done'][:T - 1].any()), "no env is done before step T - 1"
        assert (ref['t_field'] < T).any(), "no env is frozen inside the window"


def _many_tiles():
    """More tiles than workgroup slots (2 workgroups per CU at H <= 128) + 64: N 10 -> 6 envs per tile."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    E = 6 * (2 * cus + 64) + 3
    w = dict(kind='pp', env=dict(N=10, dim=5, vision=0, mode='mixed'), H=64, hard_attn=True, E=E, T=4)
    if 'many' not in _REF:
        _REF['many'] = (_play(w, False), _play(w, True), w)
    return _REF['many']


def test_more_tiles_than_workgroup_slots():
    ref, win, w = _many_tiles()
    _same(win, ref, "E = %d" % w['E'])


def test_the_window_twice_from_the_same_state_is_the_same_bits():
    _, win, w = _many_tiles()
    _same(_play(w, True), win, "second play, E = %d" % w['E'])


def test_the_window_on_the_callers_stream():
    w = CASES['tj_easy']
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        win = _play(w, True)
    side.synchronize()
    _same(win, _ref('tj_easy'), "side stream")


def test_refusals():
    from ic3net_amd import _lib, ops
    w = dict(CASES['pp'], H=256)
    env, net, fc, heads = _setup(w, 5)
    assert not ops.policy_step_window_supported(env, fc, 256)
    w = CASES['pp']
    env, net, fc, heads = _setup(w, 5)
    N, H, T = 3, 64, 2
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    args = lambda: (env, fc, H, heads, True, False, T, z(T + 1, 15, H), z(T + 1, 15, H), None, None, z(T, 15, 8),
                    z(T, 2, 5, N, dt=torch.int32), z(T, 5, N), z(T, 5, dt=torch.int32))
    env.set_hidden_out(z(15, H), z(15, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_policy_window\)"):
        ops.policy_step_window(*args())
    ops.policy_step_window(*args())                                # disarmed by the refused call
    fc32 = dict(fc, ps_l_wp3=None)
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window\)"):
        ops.policy_step_window(*((env, fc32) + args()[2:]))

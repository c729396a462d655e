"""GPU: `ic3_policy_step` on an `ic3_commnet_window` — T steps of `ic3_commnet_step` in ONE launch (the WIN instantiations of
csrc/commnet_fwd.hip) — against T per-step launches of the same library on a twin handle, BIT FOR BIT: out, action, reward, done,
alive, is_completed, all T snapshots, h slots 1 .. T of the tanh recurrence or the h_fin record, and the state the handle is left in.

The per-step side plays what the Trainer's recorded rollout plays: ic3_env_snapshot in front of the step, the masks of step t - 1
handed over.  The cases are those of tests/test_host_commnet_window_cpu.py, plus: more tiles than the device has workgroup slots (a CU
plays several tiles in turn, its vector L1 warm with the lines of the tile before — the hand-off between two steps of a workgroup
must not read them) for the narrow and the wide tile, the window twice from the same state, and the window on the caller's
non-default stream."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_env_parity_gpu import make_pp, make_tj  # noqa: E402

KEYS = ('out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'hs', 'h_fin')

CASES = {
    'pp_commnet_p2': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=64, hard_attn=True, passes=2, E=45, T=6),
    'tj_easy_commnet': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=128,
                            hard_attn=False, passes=2, E=26, T=8),
    'pp_ic_auto': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=64, hard_attn=False, passes=1, ic=True, auto=3,
                       E=45, T=7),
    'pp_tanh_done': dict(kind='pp', env=dict(N=2, dim=3, vision=1, mode='mixed'), H=64, hard_attn=False, passes=1, tanh=True, E=40, T=8),
    # (with an h_fin record beside the recurrence's own: slot t of it = slot t + 1 of h)
    'pp_tanh_auto': dict(kind='pp', env=dict(N=2, dim=3, vision=1, mode='mixed'), H=64, hard_attn=False, passes=1, tanh=True, h_fin=True,
                         auto=3, E=40, T=8),
}


def _setup(w, E, seed=7, offset=40, H=None):
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
    N, H = env.nagents_env, H or w['H']
    heads = [env.dims.naction, 2] if w['hard_attn'] else [env.dims.naction]
    torch.manual_seed(H + N)
    # (the IC stand-in and the tanh recurrence are this module with one pass and the communication block off: comm_zero below)
    net = CommNetMLP(argparse.Namespace(nagents=N, hid_size=H, comm_passes=w['passes'], recurrent=False, continuous=False,
                                        naction_heads=heads, comm_mask_zero=False, share_weights=False, comm_init='uniform',
                                        hard_attn=w['hard_attn'], comm_mode='avg', rnn_type='MLP', init_std=0.2),
                     env.obs_dim).cuda().float()
    with torch.no_grad():
        for hd in net.heads:
            hd.weight.mul_(4.0)
        net.obs_encoder, net.obs_table = env.encode, env.encode_table
        cn = net._commnet_cache()
    return env, cn, heads


def _play(w, window, E=None, T=None):
    from ic3net_amd import ops
    E, T = E or w['E'], T or w['T']
    env, cn, heads = _setup(w, E)
    N, H, dev = env.nagents_env, w['H'], env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(out=f(T, R, OT), action=i(T, nh, E, N), reward=f(T, E, N), done=i(T, E), alive=i(T, E, N), comp=i(T, E, N),
             snaps=i(T, env.dims.state_words), hs=f(T + 1, R, H), h_fin=f(T, R, H))
    b['hs'][0] = (torch.randn((R, H), generator=torch.Generator(device='cpu').manual_seed(11)) * 0.3).to(dev)
    tj, tanh, ic = w['kind'] == 'tj', bool(w.get('tanh')), bool(w.get('ic'))
    cz = tanh or ic
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else None
    with torch.no_grad():
        if window:
            assert ops.commnet_step_window_supported(env, cn, H)
            ops.commnet_step_window(env, cn, H, heads, True, cz, T, alive_in, comm_in, b['out'], b['action'], b['reward'], b['done'],
                                    b['alive'], b['comp'], hs=b['hs'] if tanh else None, h_fin=b['h_fin'] if (ic or w.get('h_fin')) else None,
                                    snaps=b['snaps'], alive_prev=tj, comm_mode='last_head' if w['hard_attn'] else 'all')
        else:
            for t in range(T):
                env.snapshot(out=b['snaps'][t])
                ops.commnet_step(env, cn, H, heads, True, cz, alive_in, comm_in, b['out'][t], b['action'][t], b['reward'][t],
                                 b['done'][t], b['alive'][t], b['comp'][t], h_in=b['hs'][t] if tanh else None,
                                 h_out=b['hs'][t + 1] if tanh else b['h_fin'][t] if ic else None)
                if tj:
                    alive_in = b['alive'][t]
                if w['hard_attn']:
                    comm_in = b['action'][t, nh - 1]
            if w.get('h_fin'):                                     # (the per-step call has one h_out: the recurrence's next slot)
                b['h_fin'].copy_(b['hs'][1:])
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['t_field'] = env.get_state()['t']
    return b


def _same(a, b, what):
    for key in KEYS + ('state',):
        x, y = a[key], b[key]
        same = torch.equal(x.view(torch.int32), y.view(torch.int32))      # bits (the records a case does not use hold NaN on both sides)
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
    assert bool(torch.isfinite(ref['out']).all()) and bool((ref['action'] >= 0).all())
    assert bool(torch.isfinite(ref['hs']).all()) == bool(w.get('tanh')) and bool(torch.isfinite(ref['h_fin']).all()) == bool(w.get('ic') or w.get('h_fin'))
    if name == 'pp_commnet_p2':
        gate = ref['action'][:, -1]
        assert bool((gate == 0).any()) and bool((gate == 1).any()), "the gate chain carries one value only"
    if w['kind'] == 'tj':
        assert bool((ref['alive'][1:] != ref['alive'][:-1]).any()), "no car's alive flag changes inside the window"
    if w.get('auto'):
        assert bool(ref['done'][:T - 1].any()), "no episode ends inside the window"
    if name == 'pp_tanh_done':
        assert bool(ref['done'][:T - 1].any()), "no env is done before step T - 1"
        assert (ref['t_field'] < T).any(), "no env is frozen inside the window"


def _many_tiles(narrow):
    """More tiles than workgroup slots (3 workgroups per CU for the narrow tile, 2 for the wide one) + 64: N 10 -> 6 envs per tile."""
    key = 'many_narrow' if narrow else 'many_wide'
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    E = 6 * (3 * cus + 64) + 3
    w = dict(kind='pp', env=dict(N=10, dim=5, vision=0, mode='mixed'), H=64, hard_attn=not narrow, passes=1, ic=narrow, E=E, T=4)
    if key not in _REF:
        _REF[key] = (_play(w, False), _play(w, True), w)
    return _REF[key]


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_more_tiles_than_workgroup_slots(narrow):
    ref, win, w = _many_tiles(narrow)
    _same(win, ref, "E = %d" % w['E'])


def test_the_window_twice_from_the_same_state_is_the_same_bits():
    _, win, w = _many_tiles(False)
    _same(_play(w, True), win, "second play, E = %d" % w['E'])


def test_the_window_on_the_callers_stream():
    w = CASES['tj_easy_commnet']
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        win = _play(w, True)
    side.synchronize()
    _same(win, _ref('tj_easy_commnet'), "side stream")


def test_refusals():
    from ic3net_amd import ops
    w = CASES['pp_tanh_done']
    env, cn, heads = _setup(w, 5, H=256)
    assert not ops.commnet_step_window_supported(env, cn, 256)
    env, cn, heads = _setup(w, 5)
    N, H, T, R = 2, 64, 2, 10
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    args = lambda: (env, cn, H, heads, True, True, T, None, None, z(T, R, 6), z(T, 1, 5, N, dt=torch.int32), z(T, 5, N),
                    z(T, 5, dt=torch.int32), None, None)
    env.set_hidden_out(z(R, H), z(R, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_commnet_window\)"):
        ops.commnet_step_window(*args(), hs=z(T + 1, R, H))
    ops.commnet_step_window(*args(), hs=z(T + 1, R, H))            # disarmed by the refused call
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_commnet_window\)"):
        ops.commnet_step_window(*((env, dict(cn, wp3=None)) + args()[2:]), hs=z(T + 1, R, H))

"""GPU: `ic3_policy_step` on an `ic3_policy_window` tagged IC3_POLICY_WINDOW_PASSES — T lock-steps of a comm_passes = 2..4 policy's
recorded training rollout in ONE launch (the MP + WIN instantiations of csrc/policy_step.hip) — against T per-step launches of the
same library (the in-launch pass loop, ic3_policy.npasses) on a twin handle, BIT FOR BIT: the (h, c) record, out, action, reward,
done, alive, is_completed, all T snapshots and the state the handle is left in.

The per-step side plays what the recorded rollout plays: ic3_env_snapshot in front of the step, ic3_env_set_hidden_out to slot t + 1
(the inner passes then hand c on through that slot, as the window does), the masks of step t - 1 handed over.  The shapes are those
of tests/test_host_policy_window_passes_cpu.py."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_env_parity_gpu import make_pp, make_tj  # noqa: E402

KEYS = ('hs', 'cs', 'out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'state')

CASES = {
    'pp_p2': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=64, hard_attn=True, E=45, T=6, passes=2),
    'tj_easy_p3_shared': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=128,
                              hard_attn=True, E=26, T=8, passes=3, shared=True),
    'pp_auto_p2': dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=64, hard_attn=False, ones=True, auto=3, E=45, T=7,
                       passes=2),
    'pp_done_p4': dict(kind='pp', env=dict(N=2, dim=3, vision=1, mode='mixed'), H=64, hard_attn=False, E=40, T=8, passes=4),
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
    net = CommNetMLP(argparse.Namespace(nagents=N, hid_size=H, comm_passes=w['passes'], recurrent=True, continuous=False,
                                        naction_heads=heads, comm_mask_zero=False, share_weights=bool(w.get('shared')),
                                        comm_init='uniform', hard_attn=w['hard_attn'], comm_mode='avg', rnn_type='LSTM', init_std=0.2),
                     env.obs_dim).cuda().float()
    with torch.no_grad():
        for hd in net.heads:
            hd.weight.mul_(4.0)
        net.obs_encoder, net.obs_table = env.encode, env.encode_table
        fc = net._fused_cache()
    return env, net, fc, heads


def _play(w, mode):
    """mode 'steps': T per-step launches of `passes` passes each; 'window': one launch; 'one_pass': the one-pass window (pass 0's C)."""
    from ic3net_amd import ops
    E, T, P = w['E'], w['T'], w['passes']
    env, net, fc, heads = _setup(w, E)
    N, H, dev = env.nagents_env, w['H'], env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(hs=f(T + 1, R, H), cs=f(T + 1, R, H), out=f(T, R, OT), action=i(T, nh, E, N), reward=f(T, E, N), done=i(T, E),
             alive=i(T, E, N), comp=i(T, E, N), snaps=i(T, env.dims.state_words))
    g = torch.Generator(device='cpu').manual_seed(11)
    b['hs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    b['cs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    tj = w['kind'] == 'tj'
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else \
        torch.ones((E, N), dtype=torch.int32, device=dev) if w.get('ones') else None
    comm_mode = 'last_head' if w['hard_attn'] else 'ones' if w.get('ones') else 'all'
    with torch.no_grad():
        if mode != 'steps':
            passes = P if mode == 'window' else 1
            assert ops.policy_step_window_supported(env, fc, H, passes=passes)
            ops.policy_step_window(env, fc, H, heads, True, False, T, b['hs'], b['cs'], alive_in, comm_in, b['out'], b['action'],
                                   b['reward'], b['done'], b['alive'], b['comp'], snaps=b['snaps'], alive_prev=tj, comm_mode=comm_mode,
                                   passes=passes)
        else:
            assert ops.policy_step_passes_supported(fc, H, P)
            for t in range(T):
                env.snapshot(out=b['snaps'][t])
                env.set_hidden_out(b['hs'][t + 1], b['cs'][t + 1])
                ops.policy_step(env, fc, H, heads, True, False, b['hs'][t], b['cs'][t], alive_in, comm_in, b['out'][t], b['action'][t],
                                b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t], passes=P)
                if tj:
                    alive_in = b['alive'][t]
                if w['hard_attn']:
                    comm_in = b['action'][t, nh - 1]
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['t_field'] = env.get_state()['t']
    return b


def _same(a, b, what):
    for key in KEYS:
        x, y = a[key].view(torch.int32), b[key].view(torch.int32)         # bits
        assert torch.equal(x, y), "%s: %s differs in %d words" % (what, key, int((x != y).sum()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_window_launch_writes_the_bits_of_T_per_step_multipass_launches(name):
    w = CASES[name]
    ref, win = _play(w, 'steps'), _play(w, 'window')
    _same(win, ref, name)
    T = w['T']
    assert bool(torch.isfinite(ref['hs']).all()) and bool(torch.isfinite(ref['cs']).all()) and bool(torch.isfinite(ref['out']).all())
    assert bool((ref['action'] >= 0).all())
    assert len({ref['snaps'][t].cpu().numpy().tobytes() for t in range(T)}) == T, "two steps of the window enter on the same state"
    assert all(bool((ref['cs'][t + 1] != ref['cs'][t]).any()) for t in range(T))
    one = _play(w, 'one_pass')                                     # the pass loop ran: one pass per step gives other rows
    assert not torch.equal(one['out'], win['out']) and not torch.equal(one['hs'][1], win['hs'][1])
    if name == 'pp_p2':
        assert sorted(ref['action'][:, -1].unique().tolist()) == [0, 1], "the last head's draws do not carry both gate values"
    if name == 'tj_easy_p3_shared':
        assert bool((ref['alive'][1:] != ref['alive'][:-1]).any()), "no car's alive flag changes inside the window"
    if name == 'pp_auto_p2':
        assert bool(ref['done'][:T - 1].any()), "no episode ends inside the window"
    if name == 'pp_done_p4':
        assert bool(ref['done'][:T - 1].any()), "no env is done before step T - 1"
        assert (ref['t_field'] < T).any(), "no env is frozen inside the window"


def test_refusals():
    from ic3net_amd import ops
    w = CASES['pp_p2']
    env, net, fc, heads = _setup(w, 5)
    N, H, T = 3, 64, 2
    assert not ops.policy_step_window_supported(env, fc, H, passes=5)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    args = lambda: (env, fc, H, heads, True, False, T, z(T + 1, 15, H), z(T + 1, 15, H), None, None, z(T, 15, 8),
                    z(T, 2, 5, N, dt=torch.int32), z(T, 5, N), z(T, 5, dt=torch.int32))
    env.set_hidden_out(z(15, H), z(15, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_policy_window, passes\)"):
        ops.policy_step_window(*args(), passes=2)
    ops.policy_step_window(*args(), passes=2)                      # disarmed by the refused call
    fc32 = dict(fc, ps_l_wp3=None)
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window, passes\)"):
        ops.policy_step_window(*((env, fc32) + args()[2:]), passes=2)

"""GPU: `ic3_policy_step` on an `ic3_policy_window` tagged IC3_POLICY_WINDOW_WIDE_PASSES — T lock-steps of a comm_passes = 2..4
policy's recorded training rollout at hid_size 256 in ONE launch (policy_step_kernel<256, PP | TJ, 1, 1, 0, 1>: one workgroup of 512
threads per CU) — against T per-step launches of the same library (the in-launch pass loop at hid 256, ic3_policy.npasses) on a twin
handle, BIT FOR BIT: the (h, c) record, out, action, reward, done, alive, is_completed, all T snapshots and the state the handle is
left in.

The per-step side plays what the recorded rollout plays: ic3_env_snapshot in front of the step, ic3_env_set_hidden_out to slot t + 1
(the inner passes then hand c on through that slot, as the window does), the masks of step t - 1 handed over.  The cases are those of
tests/test_host_policy_window_wide_passes_cpu.py at the env counts of tests/test_policy_window_passes_gpu.py's kinds, plus what only
the device has: more tiles than workgroup slots, the Predator-Prey tile of pp_scaled (N 32), the window twice from fresh handles."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_policy_window_passes_gpu import _same, _setup  # noqa: E402

H = 256
PP = dict(N=3, dim=5, vision=1, mode='mixed')
CASES = {
    'pp_p2': dict(kind='pp', env=PP, H=H, hard_attn=True, E=23, T=6, passes=2),
    'tj_easy_p3_shared': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=H,
                              hard_attn=True, E=14, T=8, passes=3, shared=True),
    'pp_auto_p2': dict(kind='pp', env=PP, H=H, hard_attn=False, ones=True, auto=3, E=23, T=7, passes=2),
    'pp_done_p4': dict(kind='pp', env=dict(N=2, dim=3, vision=1, mode='mixed'), H=H, hard_attn=False, E=40, T=8, passes=4),
    # the Predator-Prey tile of pp_scaled: 2 envs per tile, a remainder tile of one
    'pp_n32': dict(kind='pp', env=dict(N=32, dim=40, vision=2, mode='mixed'), H=H, hard_attn=True, E=5, T=2, passes=2),
}
# two windows of collection mode: episodes of 2 steps over windows of 3 (every env enters the second window mid-episode)
CONTINUE = dict(kind='pp', env=PP, H=H, hard_attn=True, auto=2, E=23, T=3, passes=2)


def _play(w, mode, nwin=1):
    """mode 'steps': nwin * T per-step launches of `passes` passes each; 'window': nwin consecutive launches under the new tag, each
    continuing the one before; 'one_pass': the one-pass wide window (pass 0's C).  One record of all slots."""
    from ic3net_amd import ops
    E, T, P = w['E'], w['T'], w['passes']
    env, net, fc, heads = _setup(w, E)
    N, dev = env.nagents_env, env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    n = nwin * T
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(hs=f(n + 1, R, H), cs=f(n + 1, R, H), out=f(n, R, OT), action=i(n, nh, E, N), reward=f(n, E, N), done=i(n, E),
             alive=i(n, E, N), comp=i(n, E, N), snaps=i(n, env.dims.state_words))
    g = torch.Generator(device='cpu').manual_seed(11)
    b['hs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    b['cs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    tj = w['kind'] == 'tj'
    ones = torch.ones((E, N), dtype=torch.int32, device=dev) if w.get('ones') else None
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else ones
    comm_mode = 'last_head' if w['hard_attn'] else 'ones' if w.get('ones') else 'all'
    after = lambda t: (b['alive'][t] if tj else None, b['action'][t, nh - 1] if w['hard_attn'] else ones)
    with torch.no_grad():
        if mode == 'one_pass':
            assert ops.policy_step_window_supported(env, fc, H, wide=True)
            ops.policy_step_window(env, fc, H, heads, True, False, T, b['hs'], b['cs'], alive_in, comm_in, b['out'], b['action'],
                                   b['reward'], b['done'], b['alive'], b['comp'], snaps=b['snaps'], alive_prev=tj, comm_mode=comm_mode,
                                   wide=True)
        elif mode == 'window':
            assert ops.policy_step_window_supported(env, fc, H, passes=P, wide_passes=True)
            assert not ops.policy_step_window_supported(env, fc, H, passes=P) and not ops.policy_step_window_supported(env, fc, H, passes=P, wide=True)
            for k in range(nwin):
                s = slice(k * T, (k + 1) * T)
                ops.policy_step_window(env, fc, H, heads, True, False, T, b['hs'][k * T:(k + 1) * T + 1], b['cs'][k * T:(k + 1) * T + 1],
                                       alive_in, comm_in, b['out'][s], b['action'][s], b['reward'][s], b['done'][s], b['alive'][s],
                                       b['comp'][s], snaps=b['snaps'][s], alive_prev=tj, comm_mode=comm_mode, passes=P, wide_passes=True)
                alive_in, comm_in = after((k + 1) * T - 1)
        else:
            assert ops.policy_step_passes_supported(fc, H, P, wide_passes=True)
            for t in range(n):
                env.snapshot(out=b['snaps'][t])
                env.set_hidden_out(b['hs'][t + 1], b['cs'][t + 1])
                ops.policy_step(env, fc, H, heads, True, False, b['hs'][t], b['cs'][t], alive_in, comm_in, b['out'][t], b['action'][t],
                                b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t], passes=P)
                alive_in, comm_in = after(t)
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['t_field'] = env.get_state()['t']
    return b


_REF = {}


def _ref(name, mode):
    if (name, mode) not in _REF:
        _REF[(name, mode)] = _play(CASES[name], mode)
    return _REF[(name, mode)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_wide_window_launch_writes_the_bits_of_T_per_step_multipass_launches(name):
    w = CASES[name]
    ref, win = _ref(name, 'steps'), _ref(name, 'window')
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


def test_two_consecutive_wide_windows_write_the_bits_of_2T_per_step_multipass_launches():
    w = CONTINUE
    T = w['T']
    ref, win = _play(w, 'steps', nwin=2), _play(w, 'window', nwin=2)
    _same(win, ref, "two windows")
    done = ref['done'].to(torch.bool)
    assert bool(done[:T - 1].any(0).all()) and bool(done[T:2 * T - 1].any(0).all()), "an env does not restart strictly inside a window"
    gate = ref['action'][T - 1, -1]
    assert bool((gate == 0).any()) and bool((gate == 1).any()), "the gate handed to the second window carries one value only"


def test_more_tiles_than_workgroup_slots():
    """ONE workgroup per CU at hid 256: tile count = CU count + 64, plus a remainder tile (N 10 -> 6 envs per tile)."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    w = dict(kind='pp', env=dict(N=10, dim=5, vision=0, mode='mixed'), H=H, hard_attn=True, E=6 * (cus + 64) + 3, T=2, passes=2)
    _same(_play(w, 'window'), _play(w, 'steps'), "E = %d" % w['E'])


def test_two_fresh_handles_from_one_seed_give_the_same_bits():
    _same(_play(CASES['pp_p2'], 'window'), _ref('pp_p2', 'window'), "second handle")


def test_refusals():
    from ic3net_amd import ops
    env, net, fc, heads = _setup(CASES['pp_p2'], 5)
    N, T = 3, 2
    assert not ops.policy_step_window_supported(env, fc, H, passes=5, wide_passes=True)
    assert not ops.policy_step_window_supported(env, fc, H, passes=1, wide_passes=True)       # (one pass: the WINDOW_WIDE tag's)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    args = lambda: (env, fc, H, heads, True, False, T, z(T + 1, 15, H), z(T + 1, 15, H), None, None, z(T, 15, 8),
                    z(T, 2, 5, N, dt=torch.int32), z(T, 5, N), z(T, 5, dt=torch.int32))
    # the narrow passes tag and the one-pass wide tag keep their answers at hid 256 with two passes
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window, passes\)"):
        ops.policy_step_window(*args(), passes=2)
    with pytest.raises(AssertionError):
        ops.policy_step_window(*args(), passes=2, wide=True)
    env.set_hidden_out(z(15, H), z(15, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_policy_window, wide passes\)"):
        ops.policy_step_window(*args(), passes=2, wide_passes=True)
    ops.policy_step_window(*args(), passes=2, wide_passes=True)    # disarmed by the refused call
    fc32 = dict(fc, ps_l_wp3=None)
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window, wide passes\)"):
        ops.policy_step_window(*((env, fc32) + args()[2:]), passes=2, wide_passes=True)
    with torch.no_grad():
        assert not net.window_supported(env) and not net.window_supported(env, wide=True)
        assert not net.window_supported(env, wide=True, wide_passes=True), "without args.passes_in_launch_wide the steps are per pass"
        net.args.passes_in_launch_wide = 1
        assert net.window_supported(env, wide=True, wide_passes=True)
        assert not net.window_supported(env, wide_passes=True) and not net.window_supported(env, wide=True)

"""GPU: `ic3_policy_step` with `ic3_policy.npasses` = 2..4 at hid_size 256 — every communication pass of the step inside ONE launch
(policy_step_kernel<256, PP | TJ, 1, 1, 0, 0>: one workgroup of 512 threads per CU) — against one launch per pass of the same library
(ops.policy_step_pass x (P - 1) + ops.policy_step) on a twin handle, BIT FOR BIT: out, action, reward, done, alive, is_completed, h, c
of every step, and the dense observation rows where the call assembles them.

The cases are those of tests/test_host_passes_in_launch_wide_cpu.py, plus what only the device has: more tiles than workgroup slots
(a CU plays a second tile; the inner passes' c hand-off goes through memory past a vector L1 that is warm with the first tile's
lines), the Predator-Prey tile of pp_scaled (N 32: 2 envs per tile), two fresh handles from one seed, and the float64 policy of
oracle.policy_ref (comm_passes = 2) on the oracle env at the project's 1e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_policy_window_passes_gpu import _setup  # noqa: E402

H = 256
TOL = 1e-5     # north_star: policy forward within 1e-5 fp32 (tests/test_host_policy_step_cpu.py)
SEED, OFFSET = 7, 40
PP = dict(N=3, dim=5, vision=1, mode='mixed')
CASES = {
    # 21 envs per 64-row tile: a full tile and a half-tile remainder; the gate chain
    'pp_p2': dict(kind='pp', env=PP, H=H, hard_attn=True, E=23, T=4, passes=2),
    # the alive slice of step t - 1 is step t's mask; every pass shares C_modules[0]; 12 envs per tile
    'tj_easy_p3_shared': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=H,
                              hard_attn=True, E=14, T=6, passes=3, shared=True),
    # auto-reset: episodes of 3 steps restart inside the run (zero state in pass 0 only); a gate of ones
    'pp_auto_p2': dict(kind='pp', env=PP, H=H, hard_attn=False, ones=True, auto=3, E=23, T=5, passes=2),
    # the pass limit; no gate at all
    'pp_p4': dict(kind='pp', env=dict(N=2, dim=3, vision=1, mode='mixed'), H=H, hard_attn=False, E=40, T=3, passes=4),
    # the Predator-Prey tile of pp_scaled: 2 envs per tile, a remainder tile of one
    'pp_n32': dict(kind='pp', env=dict(N=32, dim=40, vision=2, mode='mixed'), H=H, hard_attn=True, E=5, T=2, passes=2),
}
FIELDS = ('out', 'action', 'reward', 'done', 'alive', 'comp', 'h', 'c', 'obs')


def _play(w, one_launch, dense=False):
    """T free-running steps from the zero state; every step's outputs in one record."""
    from ic3net_amd import ops
    E, T, P = w['E'], w['T'], w['passes']
    env, net, fc, heads = _setup(w, E, seed=SEED, offset=OFFSET)
    N, dev = env.nagents_env, env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(out=f(T, R, OT), action=i(T, nh, E, N), reward=f(T, E, N), done=i(T, E), alive=i(T, E, N), comp=i(T, E, N), h=f(T, R, H),
             c=f(T, R, H), obs=f(T, E, N, env.obs_dim if dense else 1))
    h = torch.zeros((R, H), dtype=torch.float32, device=dev)
    c = torch.zeros((R, H), dtype=torch.float32, device=dev)
    tj = w['kind'] == 'tj'
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else \
        torch.ones((E, N), dtype=torch.int32, device=dev) if w.get('ones') else None
    with torch.no_grad():
        assert ops.policy_step_passes_supported(fc, H, P, wide_passes=True) and not ops.policy_step_passes_supported(fc, H, P)
        for t in range(T):
            rest = (b['out'][t], b['action'][t], b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t], b['obs'][t] if dense else None)
            if one_launch:
                ops.policy_step(env, fc, H, heads, True, False, h, c, alive_in, comm_in, *rest, passes=P)
            else:
                for k in range(P - 1):
                    ops.policy_step_pass(env, fc, H, heads, True, False, h, c, alive_in, comm_in, k)
                ops.policy_step(env, fc, H, heads, True, False, h, c, alive_in, comm_in, *rest, pass_index=P - 1)
            b['h'][t].copy_(h)
            b['c'][t].copy_(c)
            if tj:
                alive_in = b['alive'][t]
            if w['hard_attn']:
                comm_in = b['action'][t, nh - 1]
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['net'] = net
    return b


def _same(a, b, what, keys=FIELDS + ('state',)):
    for key in keys:
        x, y = a[key].view(torch.int32), b[key].view(torch.int32)         # bits
        assert torch.equal(x, y), "%s: %s differs in %d words" % (what, key, int((x != y).sum()))


_RUNS = {}


def _run(name, one_launch, dense=False):
    key = (name, one_launch, dense)
    if key not in _RUNS:
        _RUNS[key] = _play(CASES[name], one_launch, dense)
    return _RUNS[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_passes_in_one_launch_write_the_bits_of_one_launch_per_pass(name):
    w = CASES[name]
    ref, one = _run(name, False), _run(name, True)
    _same(one, ref, name)
    for key in ('out', 'h', 'c'):
        assert bool(torch.isfinite(ref[key]).all()), key
    assert bool((ref['action'] >= 0).all())
    if name == 'pp_p2':
        assert sorted(ref['action'][:, -1].unique().tolist()) == [0, 1], "the last head's draws do not carry both gate values"
    if name == 'tj_easy_p3_shared':
        assert bool((ref['alive'][1:] != ref['alive'][:-1]).any()), "no car's alive flag changes inside the run"
    if name == 'pp_auto_p2':
        assert bool(ref['done'][:w['T'] - 1].any()), "no episode ends inside the run"


def test_dense_observation_rows_come_from_the_last_pass():
    ref, one = _play(CASES['pp_p2'], False, dense=True), _run('pp_p2', True, dense=True)
    _same(one, ref, "dense obs rows")
    assert bool(torch.isfinite(ref['obs']).all()) and bool((ref['obs'] != 0).any())
    # the rows change nothing else
    _same(one, _run('pp_p2', True), "with and without obs rows", keys=FIELDS[:-1] + ('state',))


def test_more_tiles_than_workgroup_slots():
    """ONE workgroup per CU at hid 256: tile count = CU count + 64, plus a remainder tile (N 10 -> 6 envs per tile)."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    w = dict(kind='pp', env=dict(N=10, dim=5, vision=0, mode='mixed'), H=H, hard_attn=True, E=6 * (cus + 64) + 3, T=2, passes=2)
    _same(_play(w, True), _play(w, False), "E = %d" % w['E'])


def test_two_fresh_handles_from_one_seed_give_the_same_bits():
    _same(_play(CASES['pp_p2'], True), _run('pp_p2', True), "second handle")


def test_the_launch_stays_within_1e_5_of_the_float64_policy_with_two_passes():
    """The in-launch run of the Predator-Prey case with its obs rows, env by env: oracle.policy_ref.forward(comm_passes = 2) in float64
    on the oracle env, driven by the launch's own actions."""
    import oracle
    from oracle import policy_ref
    w = CASES['pp_p2']
    b = _run('pp_p2', True, dense=True)
    E, T, N = w['E'], w['T'], w['env']['N']
    params = {k: v.detach().cpu().double().numpy() for k, v in b['net'].state_dict().items()}
    rec = {k: b[k].cpu().numpy() for k in FIELDS}
    worst = 0.0
    for e in range(E):
        o = oracle.PPOracle(N, w['env']['dim'], w['env']['vision'], 'mixed', seed=SEED, env_gid=OFFSET + e)
        obs = o.reset()
        hc = (np.zeros((N, H)), np.zeros((N, H)))
        g = np.zeros(N)
        for t in range(T):
            np.testing.assert_array_equal(rec['obs'][t, e], obs, err_msg="obs rows env %d step %d" % (e, t))
            logp, val, hc = policy_ref.forward(params, obs[None].astype(np.float64), hc, None, g, recurrent=True, comm_passes=2,
                                               hard_attn=True, nheads=2)
            o3 = rec['out'][t].reshape(E, N, -1)[e]
            errs = [np.abs(logp[0][0] - o3[:, :5]).max(), np.abs(logp[1][0] - o3[:, 5:7]).max(), np.abs(val.reshape(-1) - o3[:, 7]).max(),
                    np.abs(hc[0] - rec['h'][t].reshape(E, N, H)[e]).max(), np.abs(hc[1] - rec['c'][t].reshape(E, N, H)[e]).max()]
            assert np.isfinite(errs).all(), (e, t, errs)
            worst = max([worst] + [float(x) for x in errs])
            obs, orew, _ = o.step(rec['action'][t, 0, e])
            np.testing.assert_array_equal(rec['reward'][t, e], np.asarray(orew).astype(np.float32))
            g = rec['action'][t, 1, e].astype(np.float64)
    print("worst |launch - float64| over %d envs x %d steps: %.3g" % (E, T, worst))
    assert worst < TOL, worst


def test_the_flag_sends_step_env_through_one_launch(monkeypatch):
    """CommNetMLP.step_env at hid 256 with comm_passes = 2: args.passes_in_launch_wide = 1 gives the bits of the default path."""
    from ic3net_amd import ops
    w = CASES['pp_p2']
    res, inner_calls = [], []
    inner = ops.policy_step_pass
    monkeypatch.setattr(ops, 'policy_step_pass', lambda *a, **k: (inner_calls.append(1), inner(*a, **k))[1])
    for flag in (0, 1):
        env, net, fc, heads = _setup(w, w['E'], seed=SEED, offset=OFFSET)
        net.args.passes_in_launch_wide = flag
        del inner_calls[:]
        E, N, dev = w['E'], env.nagents_env, env.device
        action = torch.full((2, E, N), -7, dtype=torch.int32, device=dev)
        reward, done = torch.zeros((E, N), device=dev), torch.zeros((E,), dtype=torch.int32, device=dev)
        hc = net.zero_hidden(E, dev)
        info = {'comm_action': torch.zeros((E, N), dtype=torch.int32, device=dev)}
        steps = []
        with torch.no_grad():
            assert net.mega_supported(env)
            for t in range(3):
                x = [torch.empty((E, N, env.obs_dim), device=dev), hc]   # (the launch reads the env's own state)
                action_out, value, hc = net.step_env(env, x, info, action, reward, done)
                steps.append(torch.cat([torch.cat([a.reshape(E * N, -1) for a in action_out], 1), value.reshape(E * N, 1), hc[0], hc[1],
                                        action.reshape(2, -1).t().float(), reward.reshape(-1, 1)], 1).clone())
                info = {'comm_action': action[1].clone()}
        res.append(torch.stack(steps))
        assert len(inner_calls) == (0 if flag else 3 * (w['passes'] - 1)), "launches of inner passes: %d" % len(inner_calls)
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))

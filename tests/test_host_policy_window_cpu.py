"""CPU: `ic3_policy_step` on an `ic3_policy_window` — T lock-steps of the recorded training rollout in ONE launch — on the host build
(tests/host: policy_step.hip unmodified behind the C ABI, `device = -1`), against T per-step calls of the same library.

Two handles are created from one seed.  One plays T per-step calls the way the Trainer's recorded rollout does: ic3_env_snapshot in
front of the step, ic3_env_set_hidden_out to slot t + 1 of the (h, c) record, ic3_env_set_record_out to the step's gate / inp rows,
the masks of step t - 1 handed over.  The other plays one window call.  Everything either writes must be the SAME BITS: the (h, c)
record, gates, inp, out, action, reward, done, alive, is_completed, all T snapshots and the state the handle is left in.  The
refusals are refused before any launch (sentinel-filled outputs stay untouched)."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostEnv, HostPolicy, check, p
from test_host_policy_step_cpu import make_params

CASES = {
    # full tiles of 21 envs plus a remainder; the gate chain (the last head's draws are the next step's gate)
    'pp': dict(env='pp', N=3, dim=5, vision=1, H=64, heads=[5, 2], hard_attn=True, E=45, T=6),
    # cars enter and leave inside the window: the alive slice of step t - 1 is step t's mask
    'tj_easy': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', H=128, heads=[2, 2], hard_attn=True, rate=0.3, E=26, T=8),
    # auto-reset: episodes of 3 steps restart inside the window; comm_action_one (a gate of ones)
    'pp_auto': dict(env='pp', N=3, dim=5, vision=1, H=64, heads=[5, 2], hard_attn=False, ones=True, auto=3, E=45, T=7),
    # lock-step, some env done (frozen) before the window ends; no gate at all
    'pp_done': dict(env='pp', N=2, dim=3, vision=1, H=64, heads=[5], hard_attn=False, E=40, T=8),
}


def _env(w, seed, offset):
    if w['env'] == 'pp':
        env = HostEnv.pp(w['N'], w['dim'], w['vision'], 'mixed', w['E'], seed=seed, offset=offset)
        env.reset()
    else:
        env = HostEnv.tj(w['N'], w['dim'], w['vision'], w['difficulty'], w['E'], seed=seed, offset=offset, add_rate_min=w['rate'],
                         add_rate_max=w['rate'])
        env.reset(0)
    if w.get('auto'):
        check(env.lib.ic3_env_set_auto_reset(env._h, w['auto']))
    return env


def _buffers(w, env, T=None):
    E, N, H, T = w['E'], w['N'], w['H'], T or w['T']
    R, OT, nh = E * N, sum(w['heads']) + 1, len(w['heads'])
    f = lambda *s: np.full(s, np.nan, np.float32)
    i = lambda *s: np.full(s, -7, np.int32)
    b = dict(hs=f(T + 1, R, H), cs=f(T + 1, R, H), gates=f(T, R, 4 * H), inp=f(T, R, 2 * H), out=f(T, R, OT), action=i(T, nh, R),
             reward=f(T, E, N), done=i(T, E), alive=i(T, E, N), comp=i(T, E, N), snaps=i(T, env.dims.state_words))
    rng = np.random.default_rng(11)
    b['hs'][0] = (rng.standard_normal((R, H)) * 0.3).astype(np.float32)     # (an auto-reset handle reads them as zero at t == 0)
    b['cs'][0] = (rng.standard_normal((R, H)) * 0.3).astype(np.float32)
    return b


def _masks0(w):
    """(alive_in, comm_in) of step 0: info is empty at t = 0; the gate starts at 0 (hard_attn) or is ones (comm_action_one)."""
    E, N = w['E'], w['N']
    comm = np.zeros((E, N), np.int32) if w['hard_attn'] else np.ones((E, N), np.int32) if w.get('ones') else None
    return None, comm


def _window_struct(pol, T, b, w, snap_words, size=None, tag=None):
    from ic3net_amd import _lib as binding
    win = binding.PolicyWindow()
    C.memmove(C.addressof(win), C.addressof(pol.struct), C.sizeof(pol.struct))
    win.struct_size = C.sizeof(win) if size is None else size
    win.inner_pass = win.WINDOW if tag is None else tag
    win.T = T
    win.alive_mode = win.ALIVE_PREV if w['env'] == 'tj' else win.ALIVE_ALL
    win.comm_mode = win.COMM_LAST_HEAD if w['hard_attn'] else win.COMM_ONES if w.get('ones') else win.COMM_ALL
    win.gates, win.inp = b['gates'].ctypes.data, b['inp'].ctypes.data
    win.snaps, win.snap_words = b['snaps'].ctypes.data, snap_words
    return win


def _call_window(env, win, b, alive_in, comm_in, obs=None):
    from ic3net_amd import _lib as binding
    return env.lib.ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(binding.Policy)), p(b['hs']), p(b['cs']), p(alive_in),
                                   p(comm_in), p(b['out']), p(b['action']), p(obs), p(b['reward']), p(b['done']), p(b['alive']),
                                   p(b['comp']), None)


def _play(w, window, seed=7, offset=40):
    env = _env(w, seed, offset)
    P = make_params(env.obs_dim, w['H'], w['heads'], seed=seed + 1)
    pol = HostPolicy(env, P, w['H'], w['heads'], gate_split=True)
    b = _buffers(w, env)
    T, nh = w['T'], len(w['heads'])
    alive_in, comm_in = _masks0(w)
    if window:
        check(_call_window(env, _window_struct(pol, T, b, w, env.dims.state_words), b, alive_in, comm_in))
    else:
        for t in range(T):
            b['snaps'][t] = env.snapshot()
            check(env.lib.ic3_env_set_hidden_out(env._h, p(b['hs'][t + 1]), p(b['cs'][t + 1])))
            check(env.lib.ic3_env_set_record_out(env._h, p(b['gates'][t]), p(b['inp'][t])))
            check(env.lib.ic3_policy_step(env._h, C.byref(pol.struct), p(b['hs'][t]), p(b['cs'][t]), p(alive_in), p(comm_in),
                                          p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]), p(b['done'][t]),
                                          p(b['alive'][t]), p(b['comp'][t]), None))
            if w['env'] == 'tj':
                alive_in = b['alive'][t]
            if w['hard_attn']:
                comm_in = b['action'][t, nh - 1]
    b['state'] = env.raw_state()
    b['fields'] = env.get_state()
    env.close()
    return b


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_window_launch_writes_the_bits_of_T_per_step_launches(name):
    w = CASES[name]
    ref, win = _play(w, False), _play(w, True)
    for key in ('hs', 'cs', 'gates', 'inp', 'out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'state'):
        np.testing.assert_array_equal(win[key], ref[key], err_msg="%s: %s" % (name, key))
    T = w['T']
    assert np.isfinite(ref['hs']).all() and np.isfinite(ref['out']).all() and (ref['action'] >= 0).all()
    assert len({ref['snaps'][t].tobytes() for t in range(T)}) == T, "two steps of the window enter on the same state"
    # the condition the case exists for, on this build's draws
    env = _env(w, 7, 40)
    t_off, t_cnt = env._field('t')
    env.close()
    if name == 'tj_easy':
        assert (ref['alive'][1:] != ref['alive'][:-1]).any(), "no car's alive flag changes inside the window"
        assert (ref['alive'] == 0).any() and (ref['alive'] == 1).any()
    if name == 'pp_auto':
        assert ref['done'][:T - 1].any(), "no episode ends inside the window"
        assert (ref['snaps'][1:, t_off:t_off + t_cnt] == 0).any(), "no env enters a step of the window at t == 0"
    if name == 'pp_done':
        assert ref['done'][:T - 1].any(), "no env is done before step T - 1"
        assert (ref['snaps'][T - 1, t_off:t_off + t_cnt] < T - 1).any(), "no env is frozen inside the window"


def _refusal_setup(H=64, gate_split=True, passes=1):
    w = dict(CASES['pp'], H=H, E=5, T=3)
    env = _env(w, 3, 9)
    P = make_params(env.obs_dim, H, w['heads'], seed=4, comm_passes=max(passes, 1))
    pol = HostPolicy(env, P, H, w['heads'], gate_split=gate_split, passes=passes)
    b = _buffers(w, env)
    return w, env, pol, b


def _untouched(env, b, before):
    for key in ('hs', 'cs', 'gates', 'inp', 'out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps'):
        np.testing.assert_array_equal(b[key], before[key], err_msg=key)
    np.testing.assert_array_equal(env.raw_state(), before['state'])


@pytest.mark.parametrize("what", ["size", "forward", "obs", "hid256", "fp32_gates", "npasses", "armed_hidden", "armed_record",
                                  "armed_events"])
def test_refusals_come_before_any_launch(what):
    w, env, pol, b = _refusal_setup(H=256 if what == "hid256" else 64, gate_split=what != "fp32_gates",
                                    passes=2 if what == "npasses" else 1)
    lib = env.lib
    before = {k: v.copy() for k, v in b.items()}
    before['state'] = env.raw_state()
    _, comm_in = _masks0(w)
    win = _window_struct(pol, w['T'], b, w, env.dims.state_words)
    want = -22
    if what == "size":
        win.struct_size = C.sizeof(win) + 8
        rc = _call_window(env, win, b, None, comm_in)
    elif what == "forward":
        from ic3net_amd import _lib as binding
        enc = np.zeros((w['E'] * w['N'], w['H']), np.float32)
        rc = lib.ic3_policy_forward(C.cast(C.byref(win), C.POINTER(binding.Policy)), p(enc), w['E'], w['N'], p(b['hs']), p(b['cs']),
                                    None, p(comm_in), p(b['out']), None)
    elif what == "obs":
        obs = np.full((w['E'], w['N'], env.obs_dim), np.nan, np.float32)
        rc = _call_window(env, win, b, None, comm_in, obs=obs)
        assert np.isnan(obs).all()
    elif what in ("hid256", "fp32_gates", "npasses"):
        want = -38
        rc = _call_window(env, win, b, None, comm_in)
    else:
        scratch = np.full((w['E'] * w['N'], 4 * w['H']), np.nan, np.float32)
        if what == "armed_hidden":
            check(lib.ic3_env_set_hidden_out(env._h, p(scratch), p(scratch[:, w['H']:])))
        elif what == "armed_record":
            check(lib.ic3_env_set_record_out(env._h, p(scratch), None))
        else:
            ev = [C.c_void_p(), C.c_void_p()]
            for e in ev:
                check(lib.ic3_event_create(C.byref(e)))
            check(lib.ic3_env_set_step_events(env._h, ev[0], ev[1]))
        rc = _call_window(env, win, b, None, comm_in)
        assert np.isnan(scratch).all()
    assert rc == want, (what, rc, lib.ic3_last_error().decode())
    msg = lib.ic3_last_error().decode()
    if what != "forward":
        assert msg.startswith("ic3_policy_step (ic3_policy_window)"), msg
    _untouched(env, b, before)
    if what.startswith("armed") and what != "armed_events":
        # disarmed: the next per-step call writes where its arguments say
        h, c = b['hs'][0].copy(), b['cs'][0].copy()
        plain = pol.step(env, h, c, None, comm_in, with_obs=False)
        assert np.isfinite(plain[0]).all() and not np.array_equal(h, b['hs'][0]) and np.isnan(scratch).all()
    if what == "armed_events":
        for e in ev:
            check(lib.ic3_event_destroy(e))
    env.close()

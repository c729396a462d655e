"""CPU: `ic3_policy_step` on an `ic3_policy_window` tagged `IC3_POLICY_WINDOW_PASSES` — T lock-steps of a comm_passes = 2..4 policy's
recorded training rollout in ONE launch — on the host build (tests/host: policy_step.hip unmodified behind the C ABI, `device = -1`),
against T per-step `npasses` calls of the same library.

Two handles are created from one seed.  One plays T per-step calls the way the recorded rollout does: ic3_env_snapshot in front of the
step, ic3_env_set_hidden_out to slot t + 1 of the (h, c) record, the masks of step t - 1 handed over; every call runs its passes inside
the launch (ic3_policy.npasses).  The other plays one window call.  Everything either writes must be the SAME BITS: the (h, c) record,
out, action, reward, done, alive, is_completed, all T snapshots and the state the handle is left in.  The refusals are refused before
any launch (sentinel-filled outputs stay untouched)."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostPolicy, check, p
from test_host_policy_step_cpu import make_params
from test_host_policy_window_cpu import _buffers, _call_window, _env, _masks0, _untouched, _window_struct

PREFIX = "ic3_policy_step (ic3_policy_window, passes)"
KEYS = ('hs', 'cs', 'out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'state')

CASES = {
    # two full tiles of 21 envs plus a remainder; the gate chain across steps (the last head's draws are the next step's gate)
    'pp_p2': dict(env='pp', N=3, dim=5, vision=1, H=64, heads=[5, 2], hard_attn=True, E=45, T=6, passes=2),
    # cars enter and leave inside the window: the alive slice of step t - 1 is step t's mask; one C module for all passes
    'tj_easy_p3_shared': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', H=128, heads=[2, 2], hard_attn=True, rate=0.3, E=26,
                              T=8, passes=3, shared=True),
    # auto-reset: episodes of 3 steps restart inside the window (zero state at pass 0 only); comm_action_one (a gate of ones)
    'pp_auto_p2': dict(env='pp', N=3, dim=5, vision=1, H=64, heads=[5, 2], hard_attn=False, ones=True, auto=3, E=45, T=7, passes=2),
    # lock-step, some env done (frozen) before the window ends; no gate at all; the pass limit
    'pp_done_p4': dict(env='pp', N=2, dim=3, vision=1, H=64, heads=[5], hard_attn=False, E=40, T=8, passes=4),
}


def _params(w, obs_dim, seed):
    P = make_params(obs_dim, w['H'], w['heads'], seed=seed, comm_passes=w['passes'])
    if w.get('shared'):                                         # share_weights: every pass runs C_modules[0]
        for i in range(1, w['passes']):
            P['C_modules.%d.weight' % i] = P['C_modules.0.weight']
            P['C_modules.%d.bias' % i] = P['C_modules.0.bias']
    return P


def _passes_struct(pol, T, b, w, snap_words, size=None, tag=None):
    """The window descriptor of the passes form: tag 5, the window's own size, no gate record."""
    from ic3net_amd import _lib as binding
    win = _window_struct(pol, T, b, w, snap_words, size=size, tag=binding.PolicyWindow.WINDOW_PASSES if tag is None else tag)
    win.gates = win.inp = None
    return win


def _play(w, mode, seed=7, offset=40):
    """mode 'steps': T per-step npasses calls; 'window': one passes window; 'one_pass': one IC3_POLICY_WINDOW window (pass 0's C)."""
    env = _env(w, seed, offset)
    P = _params(w, env.obs_dim, seed + 1)
    pol = HostPolicy(env, P, w['H'], w['heads'], gate_split=True, passes=1 if mode == 'one_pass' else w['passes'])
    b = _buffers(w, env)
    T, nh = w['T'], len(w['heads'])
    alive_in, comm_in = _masks0(w)
    if mode == 'window':
        check(_call_window(env, _passes_struct(pol, T, b, w, env.dims.state_words), b, alive_in, comm_in))
    elif mode == 'one_pass':
        check(_call_window(env, _window_struct(pol, T, b, w, env.dims.state_words), b, alive_in, comm_in))
    else:
        for t in range(T):
            b['snaps'][t] = env.snapshot()
            check(env.lib.ic3_env_set_hidden_out(env._h, p(b['hs'][t + 1]), p(b['cs'][t + 1])))
            check(env.lib.ic3_policy_step(env._h, C.byref(pol.struct), p(b['hs'][t]), p(b['cs'][t]), p(alive_in), p(comm_in),
                                          p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]), p(b['done'][t]),
                                          p(b['alive'][t]), p(b['comp'][t]), None))
            if w['env'] == 'tj':
                alive_in = b['alive'][t]
            if w['hard_attn']:
                comm_in = b['action'][t, nh - 1]
    b['state'] = env.raw_state()
    env.close()
    return b


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_window_launch_writes_the_bits_of_T_per_step_multipass_launches(name):
    w = CASES[name]
    ref, win = _play(w, 'steps'), _play(w, 'window')
    for key in KEYS:
        np.testing.assert_array_equal(win[key], ref[key], err_msg="%s: %s" % (name, key))
    T = w['T']
    assert np.isfinite(ref['hs']).all() and np.isfinite(ref['cs']).all() and np.isfinite(ref['out']).all() and (ref['action'] >= 0).all()
    assert np.isnan(win['gates']).all() and np.isnan(win['inp']).all(), "the passes form keeps no gate record"
    assert len({ref['snaps'][t].tobytes() for t in range(T)}) == T, "two steps of the window enter on the same state"
    # slot t is not clobbered by the inner passes' c hand-off (the bitwise comparison above), and the slots do differ
    assert all((ref['cs'][t + 1] != ref['cs'][t]).any() for t in range(T))
    # the pass loop ran: one pass per step on the same seed and weights gives other rows
    one = _play(w, 'one_pass')
    assert not np.array_equal(one['out'], win['out']) and not np.array_equal(one['hs'][1], win['hs'][1])
    # the condition the case exists for, on this build's draws
    env = _env(w, 7, 40)
    t_off, t_cnt = env._field('t')
    env.close()
    if name == 'pp_p2':
        assert set(np.unique(ref['action'][:, -1])) == {0, 1}, "the last head's draws do not carry both gate values"
    if name == 'tj_easy_p3_shared':
        assert (ref['alive'][1:] != ref['alive'][:-1]).any(), "no car's alive flag changes inside the window"
        assert (ref['alive'] == 0).any() and (ref['alive'] == 1).any()
    if name == 'pp_auto_p2':
        assert ref['done'][:T - 1].any(), "no episode ends inside the window"
        assert (ref['snaps'][1:, t_off:t_off + t_cnt] == 0).any(), "no env enters a step of the window at t == 0"
    if name == 'pp_done_p4':
        assert ref['done'][:T - 1].any(), "no env is done before step T - 1"
        assert (ref['snaps'][T - 1, t_off:t_off + t_cnt] < T - 1).any(), "no env is frozen inside the window"


def _refusal_setup(H=64, gate_split=True, passes=2):
    w = dict(CASES['pp_p2'], H=H, E=5, T=3, passes=passes)
    env = _env(w, 3, 9)
    P = make_params(env.obs_dim, H, w['heads'], seed=4, comm_passes=passes)
    pol = HostPolicy(env, P, H, w['heads'], gate_split=gate_split, passes=passes)
    b = _buffers(w, env)
    return w, env, pol, b


@pytest.mark.parametrize("what", ["size", "plain", "forward", "obs", "gates", "npasses1", "npasses5", "pass_index", "hid256",
                                  "fp32_gates", "armed_hidden", "armed_record", "armed_events"])
def test_refusals_come_before_any_launch(what):
    from ic3net_amd import _lib as binding
    w, env, pol, b = _refusal_setup(H=256 if what == "hid256" else 64, gate_split=what != "fp32_gates",
                                    passes=4 if what == "npasses5" else 2)
    lib = env.lib
    before = {k: v.copy() for k, v in b.items()}
    before['state'] = env.raw_state()
    _, comm_in = _masks0(w)
    win = _passes_struct(pol, w['T'], b, w, env.dims.state_words)
    want = -22
    if what == "size":
        win.struct_size = C.sizeof(win) + 8
        rc = _call_window(env, win, b, None, comm_in)
    elif what == "plain":                                       # a plain ic3_policy that carries the value 5
        pol.struct.inner_pass = binding.PolicyWindow.WINDOW_PASSES
        rc = lib.ic3_policy_step(env._h, C.byref(pol.struct), p(b['hs']), p(b['cs']), None, p(comm_in), p(b['out']), p(b['action']),
                                 None, p(b['reward']), p(b['done']), p(b['alive']), p(b['comp']), None)
    elif what == "forward":
        enc = np.zeros((w['E'] * w['N'], w['H']), np.float32)
        rc = lib.ic3_policy_forward(C.cast(C.byref(win), C.POINTER(binding.Policy)), p(enc), w['E'], w['N'], p(b['hs']), p(b['cs']),
                                    None, p(comm_in), p(b['out']), None)
    elif what == "obs":
        obs = np.full((w['E'], w['N'], env.obs_dim), np.nan, np.float32)
        rc = _call_window(env, win, b, None, comm_in, obs=obs)
        assert np.isnan(obs).all()
    elif what == "gates":
        win.gates, win.inp = b['gates'].ctypes.data, b['inp'].ctypes.data
        rc = _call_window(env, win, b, None, comm_in)
    elif what in ("npasses1", "npasses5", "pass_index", "hid256", "fp32_gates"):
        want = -38
        if what == "npasses1":
            win.npasses = 1
        elif what == "npasses5":
            win.npasses = 5
        elif what == "pass_index":
            win.pass_index = 1
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
        assert msg.startswith(PREFIX), msg
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


def test_the_one_pass_window_tag_still_refuses_two_passes():
    w, env, pol, b = _refusal_setup()
    before = {k: v.copy() for k, v in b.items()}
    before['state'] = env.raw_state()
    _, comm_in = _masks0(w)
    rc = _call_window(env, _window_struct(pol, w['T'], b, w, env.dims.state_words), b, None, comm_in)
    msg = env.lib.ic3_last_error().decode()
    assert rc == -38 and msg.startswith("ic3_policy_step (ic3_policy_window):"), (rc, msg)
    _untouched(env, b, before)
    env.close()

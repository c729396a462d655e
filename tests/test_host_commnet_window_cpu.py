"""CPU: `ic3_policy_step` on an `ic3_commnet_window` — T steps of `ic3_commnet_step` (the non-recurrent CommNet module, the IC
baseline's stand-in, the tanh recurrence) in ONE launch — on the host build (tests/host: commnet_fwd.hip unmodified behind the C ABI,
`device = -1`), against T per-step calls of the same library.

Two handles are created from one seed.  One plays T `ic3_commnet_step` calls the way the Trainer's recorded rollout does:
ic3_env_snapshot in front of the step, the masks of step t - 1 handed over, h_t of the tanh recurrence from slot t to slot t + 1 (or
the IC record's slot t as h_out).  The other plays one window call.  Everything either writes must be the SAME BITS: out, action,
reward, done, alive, is_completed, all T snapshots, h slots 1 .. T or h_fin, and the state the handle is left in.  The refusals are
refused before any launch (sentinel-filled outputs stay untouched)."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostEnv, check, p
from test_host_policy_step_cpu import commnet_weights, make_params

CASES = {
    # full tiles of 21 envs plus a remainder; the gate chain (the last head's draws are the next step's gate), two passes
    'pp_commnet_p2': dict(env='pp', N=3, dim=5, vision=1, H=64, heads=[5, 2], hard_attn=True, passes=2, E=45, T=6),
    # cars enter and leave inside the window: the alive slice of step t - 1 is step t's mask
    'tj_easy_commnet': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', H=128, heads=[2], hard_attn=False, passes=2, rate=0.3,
                            E=26, T=8),
    # the IC baseline's stand-in: one pass, the communication block off (the narrow tile), h_fin; episodes of 3 steps restart
    'pp_ic_auto': dict(env='pp', N=3, dim=5, vision=1, H=64, heads=[5], hard_attn=False, passes=1, ic=True, auto=3, E=45, T=7),
    # the tanh recurrence, lock-step: some env done (frozen) before the window ends; a random h slot 0
    'pp_tanh_done': dict(env='pp', N=2, dim=3, vision=1, H=64, heads=[5], hard_attn=False, passes=1, tanh=True, E=40, T=8),
    # ... and on an auto-reset handle: the rows of an env that starts an episode read as zero; with an h_fin record beside the
    # recurrence's own (slot t of it = slot t + 1 of h)
    'pp_tanh_auto': dict(env='pp', N=2, dim=3, vision=1, H=64, heads=[5], hard_attn=False, passes=1, tanh=True, h_fin=True, auto=3,
                         E=40, T=8),
}
OUT_KEYS = ('out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'hs', 'h_fin')


def make_env(w, seed, offset):
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


def make_weights(env, w, seed):
    """The module's parameters (f_modules next to make_params' C_modules) and the derived weights the calls stream."""
    H, heads, passes = w['H'], w['heads'], w['passes']
    P = make_params(env.obs_dim, H, heads, seed=seed, comm_passes=passes)
    rng = np.random.default_rng(seed + 100)
    for i in range(passes):
        P['f_modules.%d.weight' % i] = (rng.standard_normal((H, H)) * 0.1).astype(np.float32).astype(np.float64)
        P['f_modules.%d.bias' % i] = (rng.standard_normal(H) * 0.1).astype(np.float32).astype(np.float64)
    return commnet_weights(env.lib, P, H, heads, passes)


def buffers(w, env):
    E, N, H, T = w['E'], w['N'], w['H'], w['T']
    R, OT, nh = E * N, sum(w['heads']) + 1, len(w['heads'])
    f = lambda *s: np.full(s, np.nan, np.float32)
    i = lambda *s: np.full(s, -7, np.int32)
    b = dict(out=f(T, R, OT), action=i(T, nh, R), reward=f(T, E, N), done=i(T, E), alive=i(T, E, N), comp=i(T, E, N),
             snaps=i(T, env.dims.state_words), hs=f(T + 1, R, H), h_fin=f(T, R, H))
    # (an auto-reset handle reads the rows as zero at t == 0, a lock-step one reads them as they are)
    b['hs'][0] = (np.random.default_rng(11).standard_normal((R, H)) * 0.3).astype(np.float32)
    return b


def masks0(w):
    """(alive_in, comm_in) of step 0: info is empty at t = 0; the gate starts at 0 (hard_attn)."""
    return None, (np.zeros((w['E'], w['N']), np.int32) if w['hard_attn'] else None)


def comm_zero(w):
    return int(bool(w.get('ic') or w.get('tanh')))


def window_struct(w, cw, b, snap_words, size=None, split=True):
    from ic3net_amd import _lib as binding
    win = binding.CommnetWindow()
    if size is not None:
        win.struct_size = size
    win.inner_pass = win.WINDOW
    win.H, win.nheads, win.mode_avg, win.comm_zero, win.npasses = w['H'], len(w['heads']), 1, comm_zero(w), w['passes']
    for k, A in enumerate(w['heads']):
        win.head_sizes[k] = A
    win.enc_wt, win.enc_bias = cw['wt'].ctypes.data, cw['enc_bias'].ctypes.data
    win.head_w, win.head_b = cw['head_w'].ctypes.data, cw['head_b'].ctypes.data
    win.T, win.recurrence = w['T'], int(bool(w.get('tanh')))
    win.alive_mode = binding.PolicyWindow.ALIVE_PREV if w['env'] == 'tj' else binding.PolicyWindow.ALIVE_ALL
    win.comm_mode = binding.PolicyWindow.COMM_LAST_HEAD if w['hard_attn'] else binding.PolicyWindow.COMM_ALL
    win.wp, win.bias = cw['wp'].ctypes.data, cw['bias'].ctypes.data
    win.wp3 = cw['wp3'].ctypes.data if split else None
    win.h_fin = b['h_fin'].ctypes.data if (w.get('ic') or w.get('h_fin')) else None
    win.snaps, win.snap_words = b['snaps'].ctypes.data, snap_words
    return win


def call_window(env, win, w, b, alive_in, comm_in, obs=None):
    from ic3net_amd import _lib as binding
    return env.lib.ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(binding.Policy)), p(b['hs']) if w.get('tanh') else None, None,
                                   p(alive_in), p(comm_in), p(b['out']), p(b['action']), p(obs), p(b['reward']), p(b['done']),
                                   p(b['alive']), p(b['comp']), None)


def call_step(env, w, cw, b, t, alive_in, comm_in):
    sizes = np.array(w['heads'], np.int32)
    h_in = p(b['hs'][t]) if w.get('tanh') else None
    h_out = p(b['hs'][t + 1]) if w.get('tanh') else p(b['h_fin'][t]) if w.get('ic') else None
    return env.lib.ic3_commnet_step(env._h, p(cw['wt']), p(cw['enc_bias']), None, w['H'], w['passes'], p(cw['wp']), p(cw['wp3']),
                                    p(cw['bias']), p(cw['head_w']), p(cw['head_b']), p(sizes), len(w['heads']), 1, comm_zero(w),
                                    p(alive_in), p(comm_in), h_in, h_out, p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]),
                                    p(b['done'][t]), p(b['alive'][t]), p(b['comp'][t]), None)


def play(w, window, seed=7, offset=40):
    env = make_env(w, seed, offset)
    cw = make_weights(env, w, seed + 1)
    b = buffers(w, env)
    T, nh = w['T'], len(w['heads'])
    alive_in, comm_in = masks0(w)
    if window:
        check(call_window(env, window_struct(w, cw, b, env.dims.state_words), w, b, alive_in, comm_in))
    else:
        for t in range(T):
            b['snaps'][t] = env.snapshot()
            check(call_step(env, w, cw, b, t, alive_in, comm_in))
            if w['env'] == 'tj':
                alive_in = b['alive'][t]
            if w['hard_attn']:
                comm_in = b['action'][t, nh - 1]
        if w.get('h_fin'):                                         # (the per-step call has one h_out: the recurrence's next slot)
            b['h_fin'][:] = b['hs'][1:]
    b['state'] = env.raw_state()
    env.close()
    return b


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_window_launch_writes_the_bits_of_T_per_step_launches(name):
    w = CASES[name]
    ref, win = play(w, False), play(w, True)
    for key in OUT_KEYS + ('state',):
        np.testing.assert_array_equal(win[key], ref[key], err_msg="%s: %s" % (name, key))
    T = w['T']
    assert np.isfinite(ref['out']).all() and (ref['action'] >= 0).all()
    assert np.isfinite(ref['hs']).all() if w.get('tanh') else np.isnan(ref['hs'][1:]).all()
    assert np.isfinite(ref['h_fin']).all() if (w.get('ic') or w.get('h_fin')) else np.isnan(ref['h_fin']).all()
    assert len({ref['snaps'][t].tobytes() for t in range(T)}) == T, "two steps of the window enter on the same state"
    # the condition the case exists for, on the per-step side's draws
    env = make_env(w, 7, 40)
    t_off, t_cnt = env._field('t')
    env.close()
    tsteps = ref['snaps'][:, t_off:t_off + t_cnt]
    if name == 'pp_commnet_p2':
        gate = ref['action'][:, -1]
        assert (gate == 0).any() and (gate == 1).any(), "the gate chain carries one value only"
    if w['env'] == 'tj':
        assert (ref['alive'][1:] != ref['alive'][:-1]).any(), "no car's alive flag changes inside the window"
        assert (ref['alive'] == 0).any() and (ref['alive'] == 1).any()
    if w.get('auto'):
        assert ref['done'][:T - 1].any(), "no episode ends inside the window"
        assert (tsteps[1:] == 0).any(), "no env enters a step of the window at t == 0"
    if name == 'pp_tanh_done':
        assert ref['done'][:T - 1].any(), "no env is done before step T - 1"
        assert (tsteps[T - 1] < T - 1).any(), "no env is frozen inside the window"


def refusal_setup(H=64):
    w = dict(CASES['pp_tanh_done'], H=H, E=5, T=3)
    env = make_env(w, 3, 9)
    cw = make_weights(env, w, 4)
    return w, env, cw, buffers(w, env)


@pytest.mark.parametrize("what", ["size", "plain_tag", "obs", "hid256", "fp32_product", "lstm_fields", "armed_hidden"])
def test_refusals_come_before_any_launch(what):
    from ic3net_amd import _lib as binding
    w, env, cw, b = refusal_setup(H=256 if what == "hid256" else 64)
    lib = env.lib
    before = {k: v.copy() for k, v in b.items()}
    state = env.raw_state()
    win = window_struct(w, cw, b, env.dims.state_words, split=what != "fp32_product")
    want = -22
    scratch = np.full((w['E'] * w['N'], w['H']), np.nan, np.float32)
    if what == "size":
        win.struct_size = C.sizeof(win) + 8
    elif what == "plain_tag":
        win.struct_size = C.sizeof(binding.Policy)               # a plain ic3_policy that carries the value 4
    elif what in ("hid256", "fp32_product"):
        want = -38
    elif what == "lstm_fields":
        win.lstm_bias = scratch.ctypes.data
    elif what == "armed_hidden":
        check(lib.ic3_env_set_hidden_out(env._h, p(scratch), p(scratch)))
    obs = np.full((w['E'], w['N'], env.obs_dim), np.nan, np.float32) if what == "obs" else None
    rc = call_window(env, win, w, b, None, None, obs=obs)
    msg = lib.ic3_last_error().decode()
    assert rc == want, (what, rc, msg)
    assert msg.startswith("ic3_policy_step (ic3_commnet_window)"), msg
    assert obs is None or np.isnan(obs).all()
    for key in OUT_KEYS:
        np.testing.assert_array_equal(b[key], before[key], err_msg=key)
    np.testing.assert_array_equal(env.raw_state(), state)
    assert np.isnan(scratch).all()
    if what == "armed_hidden":
        check(call_window(env, win, w, b, None, None))           # disarmed: the next call passes and writes its own record
        assert np.isfinite(b['hs']).all() and np.isfinite(b['out']).all() and np.isnan(scratch).all()
    env.close()

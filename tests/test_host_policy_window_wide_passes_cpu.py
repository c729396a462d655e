"""CPU: `ic3_policy_step` on an `ic3_policy_window` tagged `IC3_POLICY_WINDOW_WIDE_PASSES` — T lock-steps of a comm_passes = 2..4
policy's recorded training rollout at hid_size 256 in ONE launch (policy_step_kernel<256, PP | TJ, 1, 1, 0, 1>) — on the host build
(tests/host: policy_step.hip unmodified behind the C ABI, `device = -1`), against T per-step `npasses` calls of the same library at
hid_size 256.

The harness is that of tests/test_host_policy_window_passes_cpu.py (its helpers are imported): two handles from one seed, one plays
per-step calls the way the recorded rollout does (ic3_env_snapshot in front of the step, ic3_env_set_hidden_out to slot t + 1, the
masks of step t - 1 handed over), the other one window call — or two consecutive ones, the second continuing the first's streams.
Everything either writes must be the SAME BITS: the (h, c) record, out, action, reward, done, alive, is_completed, all snapshots and
the state the handle is left in.  The refusals are refused before any launch (sentinel-filled outputs stay untouched).

A pass of a tile costs a second or two on the host at this width (512 emulated lanes, K = 512): the Predator-Prey case keeps a full
tile and a remainder tile, the others play one short tile; T <= 5."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostPolicy, check, p
from test_host_policy_step_cpu import make_params
from test_host_policy_window_cpu import _buffers, _call_window, _env, _masks0, _untouched, _window_struct
from test_host_policy_window_passes_cpu import _params, _passes_struct

H = 256
PREFIX = "ic3_policy_step (ic3_policy_window, wide passes)"
KEYS = ('hs', 'cs', 'out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'state')

CASES = {
    # 21 envs per 64-row tile: a full tile plus a remainder; the gate chain across steps (the last head's draws are the next step's gate)
    'pp_p2': dict(env='pp', N=3, dim=5, vision=1, H=H, heads=[5, 2], hard_attn=True, E=23, T=3, passes=2),
    # cars enter and leave inside the window: the alive slice of step t - 1 is step t's mask; one C module for all passes
    'tj_easy_p3_shared': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', H=H, heads=[2, 2], hard_attn=True, rate=0.3, E=4,
                              T=4, passes=3, shared=True),
    # auto-reset: episodes of 3 steps restart inside the window (zero state at pass 0 only); comm_action_one (a gate of ones)
    'pp_auto_p2': dict(env='pp', N=3, dim=5, vision=1, H=H, heads=[5, 2], hard_attn=False, ones=True, auto=3, E=4, T=5, passes=2),
    # lock-step, some env done (frozen) before the window ends (a 2 x 2 grid: predators meet the prey by step 2); no gate at all; the
    # pass limit
    'pp_done_p4': dict(env='pp', N=2, dim=2, vision=1, H=H, heads=[5], hard_attn=False, E=12, T=5, passes=4),
}
# two windows of collection mode: episodes of 2 steps over windows of 3 — every env restarts strictly inside both windows and enters the
# second one mid-episode (t = 1), so its step 0 reads the masks and the state it is handed
CONTINUE = dict(env='pp', N=3, dim=5, vision=1, H=H, heads=[5, 2], hard_attn=True, auto=2, E=4, T=3, passes=2)


def _wide_struct(pol, T, b, w, snap_words, **kw):
    from ic3net_amd import _lib as binding
    return _passes_struct(pol, T, b, w, snap_words, tag=binding.PolicyWindow.WINDOW_WIDE_PASSES, **kw)


def _slots(b, lo, hi):
    """The slots [lo, hi) of a record as a record of its own (views; the (h, c) record with its one slot more)."""
    return {k: (v[lo:hi + 1] if k in ('hs', 'cs') else v[lo:hi]) for k, v in b.items()}


def _play(w, mode, nwin=1, seed=7, offset=40):
    """mode 'steps': nwin * T per-step npasses calls; 'window': nwin consecutive windows under tag 8, each continuing the one before
    (its masks, its slot T as slot 0); 'one_pass': one IC3_POLICY_WINDOW_WIDE window (pass 0's C).  One record of all slots."""
    from ic3net_amd import _lib as binding
    env = _env(w, seed, offset)
    P = _params(w, env.obs_dim, seed + 1)
    pol = HostPolicy(env, P, H, w['heads'], gate_split=True, passes=1 if mode == 'one_pass' else w['passes'])
    T, nh = w['T'], len(w['heads'])
    b = _buffers(w, env, T=nwin * T)
    alive_in, comm_in = _masks0(w)

    def after(t):
        return (b['alive'][t] if w['env'] == 'tj' else None, b['action'][t, nh - 1] if w['hard_attn'] else comm_in)

    if mode == 'one_pass':
        win = _window_struct(pol, T, b, w, env.dims.state_words, tag=binding.PolicyWindow.WINDOW_WIDE)
        win.gates = win.inp = None
        check(_call_window(env, win, b, alive_in, comm_in))
    elif mode == 'window':
        for k in range(nwin):
            s = _slots(b, k * T, (k + 1) * T)
            check(_call_window(env, _wide_struct(pol, T, s, w, env.dims.state_words), s, alive_in, comm_in))
            alive_in, comm_in = after((k + 1) * T - 1)
    else:
        for t in range(nwin * T):
            b['snaps'][t] = env.snapshot()
            check(env.lib.ic3_env_set_hidden_out(env._h, p(b['hs'][t + 1]), p(b['cs'][t + 1])))
            check(env.lib.ic3_policy_step(env._h, C.byref(pol.struct), p(b['hs'][t]), p(b['cs'][t]), p(alive_in), p(comm_in),
                                          p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]), p(b['done'][t]),
                                          p(b['alive'][t]), p(b['comp'][t]), None))
            alive_in, comm_in = after(t)
    b['state'] = env.raw_state()
    t_off, t_cnt = env._field('t')
    b['tsteps'] = b['snaps'][:, t_off:t_off + t_cnt]
    env.close()
    return b


def _same(win, ref, what):
    for key in KEYS:
        np.testing.assert_array_equal(win[key], ref[key], err_msg="%s: %s" % (what, key))
    n = ref['out'].shape[0]
    assert np.isfinite(ref['hs']).all() and np.isfinite(ref['cs']).all() and np.isfinite(ref['out']).all() and (ref['action'] >= 0).all()
    assert np.isnan(win['gates']).all() and np.isnan(win['inp']).all(), "the passes form keeps no gate record"
    assert len({ref['snaps'][t].tobytes() for t in range(n)}) == n, "two steps enter on the same state"
    # slot t is not clobbered by the inner passes' c hand-off (the bitwise comparison above), and the slots do differ
    assert all((ref['cs'][t + 1] != ref['cs'][t]).any() for t in range(n))


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_wide_window_launch_writes_the_bits_of_T_per_step_multipass_launches(name):
    w = CASES[name]
    ref, win = _play(w, 'steps'), _play(w, 'window')
    _same(win, ref, name)
    T = w['T']
    # the pass loop ran: one pass per step on the same seed and weights gives other rows
    one = _play(w, 'one_pass')
    assert not np.array_equal(one['out'], win['out']) and not np.array_equal(one['hs'][1], win['hs'][1])
    # the condition the case exists for, on this build's draws
    if name == 'pp_p2':
        assert w['E'] > 64 // w['N'] and w['E'] % (64 // w['N']), "a full tile plus a remainder tile"
        assert set(np.unique(ref['action'][:, -1])) == {0, 1}, "the last head's draws do not carry both gate values"
    if name == 'tj_easy_p3_shared':
        assert (ref['alive'][1:] != ref['alive'][:-1]).any(), "no car's alive flag changes inside the window"
        assert (ref['alive'] == 0).any() and (ref['alive'] == 1).any()
    if name == 'pp_auto_p2':
        assert ref['done'][:T - 1].any(), "no episode ends inside the window"
        assert (ref['tsteps'][1:] == 0).any(), "no env enters a step of the window at t == 0"
    if name == 'pp_done_p4':
        assert ref['done'][:T - 1].any(), "no env is done before step T - 1"
        assert (ref['tsteps'][T - 1] < T - 1).any(), "no env is frozen inside the window"


def test_two_consecutive_wide_windows_write_the_bits_of_2T_per_step_multipass_calls():
    """What collection mode plays (tests/test_host_window_continue_cpu.py at 64 / 128): the second window's step 0 is handed the first
    one's last masks and its slot T as slot 0, keep_state, and reads them for every env that is mid-episode there."""
    w = CONTINUE
    T = w['T']
    ref, win = _play(w, 'steps', nwin=2), _play(w, 'window', nwin=2)
    _same(win, ref, "continue")
    done = ref['done'].astype(bool)
    for k in (0, 1):
        assert done[k * T:(k + 1) * T - 1].any(0).all(), "window %d: an env does not restart strictly inside the window" % k
    assert (ref['tsteps'][1:T] == 0).any(), "no env enters a step of the first window at t == 0"
    assert (ref['tsteps'][T] != 0).any(), "every env enters the second window at t == 0: its step 0 would not read what it is handed"
    gate = ref['action'][T - 1, -1]
    assert (gate == 0).any() and (gate == 1).any(), "the gate handed to the second window carries one value only"


def _refusal_setup(hid=H, gate_split=True, passes=2):
    w = dict(CASES['pp_p2'], H=hid, E=5, T=2, passes=passes)
    env = _env(w, 3, 9)
    P = make_params(env.obs_dim, hid, w['heads'], seed=4, comm_passes=passes)
    pol = HostPolicy(env, P, hid, w['heads'], gate_split=gate_split, passes=passes)
    b = _buffers(w, env)
    return w, env, pol, b


@pytest.mark.parametrize("what", ["hid64", "hid128", "npasses1", "npasses5", "pass_index", "fp32_gates", "gates", "obs", "size", "plain",
                                  "armed_hidden", "armed_record", "armed_events"])
def test_wide_passes_refusals_come_before_any_launch(what):
    from ic3net_amd import _lib as binding
    hid = 64 if what == "hid64" else 128 if what == "hid128" else H
    w, env, pol, b = _refusal_setup(hid=hid, gate_split=what != "fp32_gates", passes=4 if what == "npasses5" else 2)
    lib = env.lib
    before = {k: v.copy() for k, v in b.items()}
    before['state'] = env.raw_state()
    _, comm_in = _masks0(w)
    win = _wide_struct(pol, w['T'], b, w, env.dims.state_words)
    want, obs = -22, None
    scratch = np.full((w['E'] * w['N'], 4 * hid), np.nan, np.float32)
    if what in ("hid64", "hid128", "npasses1", "npasses5", "pass_index", "fp32_gates"):
        want = -38
        if what == "npasses1":
            win.npasses = 1
        elif what == "npasses5":
            win.npasses = 5
        elif what == "pass_index":
            win.pass_index = 1
    elif what == "gates":
        win.gates, win.inp = b['gates'].ctypes.data, b['inp'].ctypes.data
    elif what == "obs":
        obs = np.full((w['E'], w['N'], env.obs_dim), np.nan, np.float32)
    elif what == "size":
        win.struct_size = C.sizeof(win) + 8
    elif what == "plain":                                       # a plain ic3_policy that carries the value 8
        win.struct_size = C.sizeof(binding.Policy)
    elif what == "armed_hidden":
        check(lib.ic3_env_set_hidden_out(env._h, p(scratch), p(scratch[:, hid:])))
    elif what == "armed_record":
        check(lib.ic3_env_set_record_out(env._h, p(scratch), None))
    else:
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            check(lib.ic3_event_create(C.byref(e)))
        check(lib.ic3_env_set_step_events(env._h, ev[0], ev[1]))
    rc = _call_window(env, win, b, None, comm_in, obs=obs)
    msg = lib.ic3_last_error().decode()
    assert rc == want, (what, rc, msg)
    assert msg.startswith(PREFIX), msg
    if what in ("hid64", "hid128"):
        assert msg.count("IC3_POLICY_WINDOW_PASSES") >= 1, "the message does not name the narrow tag: " + msg
    assert obs is None or np.isnan(obs).all()
    _untouched(env, b, before)
    assert np.isnan(scratch).all()
    if what in ("armed_hidden", "armed_record"):
        # disarmed: the next window writes where its arguments say
        check(_call_window(env, _wide_struct(pol, w['T'], b, w, env.dims.state_words), b, None, comm_in))
        assert np.isfinite(b['hs'][1:]).all() and np.isfinite(b['out']).all() and np.isnan(scratch).all()
    if what == "armed_events":
        for e in ev:
            check(lib.ic3_event_destroy(e))
    env.close()


def test_the_narrow_passes_tag_and_the_one_pass_wide_tag_still_refuse_two_passes_at_hid_256():
    from ic3net_amd import _lib as binding
    w, env, pol, b = _refusal_setup()
    before = {k: v.copy() for k, v in b.items()}
    before['state'] = env.raw_state()
    _, comm_in = _masks0(w)
    for tag, prefix in ((binding.PolicyWindow.WINDOW_PASSES, "ic3_policy_step (ic3_policy_window, passes):"),
                        (binding.PolicyWindow.WINDOW_WIDE, "ic3_policy_step (ic3_policy_window, wide):")):
        rc = _call_window(env, _passes_struct(pol, w['T'], b, w, env.dims.state_words, tag=tag), b, None, comm_in)
        msg = env.lib.ic3_last_error().decode()
        assert rc == -38 and msg.startswith(prefix), (rc, msg)
        _untouched(env, b, before)
    env.close()

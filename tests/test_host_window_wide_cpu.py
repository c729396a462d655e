"""CPU: the windows at hid 256 — `ic3_policy_step` on an `ic3_policy_window` tagged IC3_POLICY_WINDOW_WIDE and on an
`ic3_commnet_window` tagged IC3_COMMNET_WINDOW_WIDE — on the host build (tests/host: the .hip sources unmodified behind the C ABI,
`device = -1`), against per-step calls of the same library.

Two handles are created from one seed.  One plays T per-step calls the way the Trainer's recorded rollout does (ic3_env_snapshot in
front of the step; the LSTM policy: ic3_env_set_hidden_out to slot t + 1, ic3_env_set_record_out to the step's gate / inp rows — at
hid 256 the inp rows alone, row stride H; ic3_commnet_step's families: h_out = the next slot of the recurrence or the step's slot of
h_fin; the masks of step t - 1 handed over).  The other plays one window call, or two consecutive ones.  Everything either writes must
be the SAME BITS: every record, out, action, reward, done, alive, is_completed, all snapshots and the state the handle is left in.
The refusals are refused before any launch (sentinel-filled outputs stay untouched).

512 emulated lanes per tile and K = 512 make one step of one tile cost one to two seconds on the host where the kernel has matrix
loops over K (the LSTM policy, the two-pass module).  Those two families therefore keep the full env count — a full and a ragged tile,
21 envs per 64-row tile — in the `pp` case only and play the other cases on one short tile (SMALL_E envs); T stays what it is.  The
IC baseline and the tanh recurrence play every case at the full env count."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostPolicy, check, p
from test_host_commnet_window_cpu import make_weights
from test_host_policy_step_cpu import make_params
from test_host_policy_window_cpu import _env

H = 256
CASES = {
    # 21 envs per 64-row tile: one full and one ragged tile; the gate chain (hard_attn: the last head's draws are the next step's gate)
    'pp': dict(env='pp', N=3, dim=5, vision=1, H=H, heads=[5, 2], hard_attn=True, E=23, T=3),
    # cars enter and leave inside the window (IC3_WINDOW_ALIVE_PREV); a gate of ones (IC3_WINDOW_COMM_ONES); 12 envs per tile
    'tj_easy': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', H=H, heads=[2, 2], hard_attn=False, ones=True, rate=0.3, E=14, T=4),
    # auto-reset: episodes of 2 steps restart inside the window
    'pp_auto': dict(env='pp', N=3, dim=5, vision=1, H=H, heads=[5, 2], hard_attn=True, auto=2, E=23, T=5),
}
# what each family records beside out / action / reward / done / alive / is_completed / snaps
FAMILIES = {'lstm': ('hs', 'cs', 'gates', 'inp'), 'commnet': (), 'ic': ('h_fin',), 'tanh': ('hs',)}
COMMON = ('out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps')
ALL_RECORDS = ('hs', 'cs', 'gates', 'inp', 'h_fin')
SMALL_E = {'tj_easy': 4, 'pp_auto': 4}       # envs of the slow families (see above) outside the two-tile case


def _case(name, family):
    w = CASES[name]
    return dict(w, E=SMALL_E[name]) if family in ('lstm', 'commnet') and name in SMALL_E else w


def _buffers(w, env, n):
    """Sentinel-filled outputs of n slots; slot 0 of the state records holds noise (an auto-reset handle reads it as zero at t == 0)."""
    E, N = w['E'], w['N']
    R, OT, nh = E * N, sum(w['heads']) + 1, len(w['heads'])
    f = lambda *s: np.full(s, np.nan, np.float32)
    i = lambda *s: np.full(s, -7, np.int32)
    # (inp: the inp rows alone — ic3_env_set_record_out's layout at hid 256)
    b = dict(hs=f(n + 1, R, H), cs=f(n + 1, R, H), gates=f(n, R, 4 * H), inp=f(n, R, H), h_fin=f(n, R, H), out=f(n, R, OT),
             action=i(n, nh, R), reward=f(n, E, N), done=i(n, E), alive=i(n, E, N), comp=i(n, E, N), snaps=i(n, env.dims.state_words))
    rng = np.random.default_rng(11)
    b['hs'][0] = (rng.standard_normal((R, H)) * 0.3).astype(np.float32)
    b['cs'][0] = (rng.standard_normal((R, H)) * 0.3).astype(np.float32)
    return b


def _gate_const(w):
    return np.ones((w['E'], w['N']), np.int32) if w.get('ones') else None


def _masks0(w):
    """(alive_in, comm_in) of the step that starts the rollout: info is empty; the gate starts at 0 (hard_attn) or is ones."""
    return None, (np.zeros((w['E'], w['N']), np.int32) if w['hard_attn'] else _gate_const(w))


def _masks_after(w, b, t):
    """(alive_in, comm_in) the Trainer hands over behind step t."""
    return (b['alive'][t] if w['env'] == 'tj' else None,
            b['action'][t, len(w['heads']) - 1].reshape(w['E'], w['N']) if w['hard_attn'] else _gate_const(w))


def _modes(w):
    from ic3net_amd import _lib as binding
    W = binding.PolicyWindow
    return (W.ALIVE_PREV if w['env'] == 'tj' else W.ALIVE_ALL,
            W.COMM_LAST_HEAD if w['hard_attn'] else W.COMM_ONES if w.get('ones') else W.COMM_ALL)


def _call(env, win, b, hs, cs, alive_in, comm_in, obs=None):
    from ic3net_amd import _lib as binding
    return env.lib.ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(binding.Policy)), hs, cs, p(alive_in), p(comm_in), p(b['out']),
                                   p(b['action']), p(obs), p(b['reward']), p(b['done']), p(b['alive']), p(b['comp']), None)


class _Lstm(object):
    """ic3_policy_step per step / on an ic3_policy_window tagged IC3_POLICY_WINDOW_WIDE."""

    def __init__(self, w, env, seed, hid=H, gate_split=True):
        self.w = w
        P = make_params(env.obs_dim, hid, w['heads'], seed=seed)
        self.pol = HostPolicy(env, P, hid, w['heads'], gate_split=gate_split)

    def step(self, env, b, t, alive_in, comm_in):
        check(env.lib.ic3_env_set_hidden_out(env._h, p(b['hs'][t + 1]), p(b['cs'][t + 1])))
        check(env.lib.ic3_env_set_record_out(env._h, p(b['gates'][t]), p(b['inp'][t])))
        check(env.lib.ic3_policy_step(env._h, C.byref(self.pol.struct), p(b['hs'][t]), p(b['cs'][t]), p(alive_in), p(comm_in),
                                      p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]), p(b['done'][t]), p(b['alive'][t]),
                                      p(b['comp'][t]), None))

    def struct(self, env, b, T):
        from ic3net_amd import _lib as binding
        win = binding.PolicyWindow()
        C.memmove(C.addressof(win), C.addressof(self.pol.struct), C.sizeof(self.pol.struct))
        win.struct_size, win.inner_pass = C.sizeof(win), win.WINDOW_WIDE
        win.T = T
        win.alive_mode, win.comm_mode = _modes(self.w)
        win.gates, win.inp = b['gates'].ctypes.data, b['inp'].ctypes.data
        win.snaps, win.snap_words = b['snaps'].ctypes.data, env.dims.state_words
        return win

    def window(self, env, b, T, alive_in, comm_in, win=None, obs=None):
        return _call(env, win or self.struct(env, b, T), b, p(b['hs']), p(b['cs']), alive_in, comm_in, obs)


class _Commnet(object):
    """ic3_commnet_step per step / on an ic3_commnet_window tagged IC3_COMMNET_WINDOW_WIDE.  kind 'commnet': two passes, the
    communication block on; 'ic': one pass, the block off (the narrow tile), an h_fin record; 'tanh': the recurrence through hs."""

    def __init__(self, w, env, seed, kind, hid=H):
        self.kind, self.tanh, self.zero = kind, kind == 'tanh', int(kind != 'commnet')
        self.w = dict(w, H=hid, passes=2 if kind == 'commnet' else 1)
        self.cw = make_weights(env, self.w, seed)
        self.sizes = np.array(w['heads'], np.int32)

    def step(self, env, b, t, alive_in, comm_in):
        w, cw = self.w, self.cw
        h_in = p(b['hs'][t]) if self.tanh else None
        h_out = p(b['hs'][t + 1]) if self.tanh else p(b['h_fin'][t]) if self.kind == 'ic' else None
        check(env.lib.ic3_commnet_step(env._h, p(cw['wt']), p(cw['enc_bias']), None, w['H'], w['passes'], p(cw['wp']), p(cw['wp3']),
                                       p(cw['bias']), p(cw['head_w']), p(cw['head_b']), p(self.sizes), len(w['heads']), 1, self.zero,
                                       p(alive_in), p(comm_in), h_in, h_out, p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]),
                                       p(b['done'][t]), p(b['alive'][t]), p(b['comp'][t]), None))

    def struct(self, env, b, T, split=True):
        from ic3net_amd import _lib as binding
        w, cw = self.w, self.cw
        win = binding.CommnetWindow()
        win.inner_pass = win.WINDOW_WIDE
        win.H, win.nheads, win.mode_avg, win.comm_zero, win.npasses = w['H'], len(w['heads']), 1, self.zero, w['passes']
        for k, A in enumerate(w['heads']):
            win.head_sizes[k] = A
        win.enc_wt, win.enc_bias = cw['wt'].ctypes.data, cw['enc_bias'].ctypes.data
        win.head_w, win.head_b = cw['head_w'].ctypes.data, cw['head_b'].ctypes.data
        win.T, win.recurrence = T, int(self.tanh)
        win.alive_mode, win.comm_mode = _modes(w)
        win.wp, win.bias = cw['wp'].ctypes.data, cw['bias'].ctypes.data
        win.wp3 = cw['wp3'].ctypes.data if split else None
        win.h_fin = b['h_fin'].ctypes.data if self.kind == 'ic' else None
        win.snaps, win.snap_words = b['snaps'].ctypes.data, env.dims.state_words
        return win

    def window(self, env, b, T, alive_in, comm_in, win=None, obs=None):
        return _call(env, win or self.struct(env, b, T), b, p(b['hs']) if self.tanh else None, None, alive_in, comm_in, obs)


def _family(w, env, family, seed):
    return _Lstm(w, env, seed) if family == 'lstm' else _Commnet(w, env, seed, family)


def _play_steps(w, family, n, seed=7, offset=40):
    """n per-step calls on one handle, their slots in one record of n (+ 1) slots."""
    env = _env(w, seed, offset)
    fam = _family(w, env, family, seed + 1)
    b = _buffers(w, env, n)
    alive_in, comm_in = _masks0(w)
    for t in range(n):
        b['snaps'][t] = env.snapshot()
        fam.step(env, b, t, alive_in, comm_in)
        alive_in, comm_in = _masks_after(w, b, t)
    b['state'] = env.raw_state()
    env.close()
    return b


def _play_windows(w, family, nwin, seed=7, offset=40):
    """nwin consecutive window calls of T steps on one handle, each into a record of its own; a window continues the one before.
    Returns them joined to the shape of _play_steps' record."""
    T = w['T']
    env = _env(w, seed, offset)
    fam = _family(w, env, family, seed + 1)
    recs, masks = [], _masks0(w)
    for k in range(nwin):
        b = _buffers(w, env, T)
        if recs:
            b['hs'][0], b['cs'][0] = recs[-1]['hs'][T], recs[-1]['cs'][T]   # (NaN where the family keeps no such record)
        check(fam.window(env, b, T, *masks))
        masks = _masks_after(w, b, T - 1)
        recs.append(b)
    out = {k: np.concatenate([r[k][:T] for r in recs[:-1]] + [recs[-1][k]]) for k in recs[0]}
    out['state'] = env.raw_state()
    env.close()
    return out


def _t_field(w):
    env = _env(w, 7, 40)
    t_off, t_cnt = env._field('t')
    env.close()
    return slice(t_off, t_off + t_cnt)


def _compare(w, family, ref, win, label):
    for key in COMMON + FAMILIES[family] + ('state',):
        np.testing.assert_array_equal(win[key], ref[key], err_msg="%s %s: %s" % (label, family, key))
    for key in set(ALL_RECORDS) - set(FAMILIES[family]) - {'hs', 'cs'}:
        assert np.isnan(win[key]).all() and np.isnan(ref[key]).all(), "%s: a record this family does not keep was written" % key
    for key in FAMILIES[family]:
        assert np.isfinite(ref[key][1:] if key in ('hs', 'cs') else ref[key]).all(), key
    assert np.isfinite(ref['out']).all() and (ref['action'] >= 0).all()
    n = ref['out'].shape[0]
    assert len({ref['snaps'][t].tobytes() for t in range(n)}) == n, "two steps enter on the same state"


# (pp_auto for the two slow families: the first window of the continuation test below IS that case — the same handle, seed, T and
#  comparison — so it is not played a second time)
@pytest.mark.parametrize("name,family", [(n, f) for n in sorted(CASES) for f in sorted(FAMILIES)
                                         if not (n == 'pp_auto' and f in ('lstm', 'commnet'))])
def test_one_wide_window_writes_the_bits_of_T_per_step_launches(name, family):
    w = _case(name, family)
    T = w['T']
    ref, win = _play_steps(w, family, T), _play_windows(w, family, 1)
    _compare(w, family, ref, win, name)
    if w is CASES[name]:
        assert (w['E'] * w['N'] + 63) // 64 >= 2 and (w['E'] % (64 // w['N'])) != 0, "one full and one ragged tile"
    # the condition the case exists for, on the per-step side's draws
    tsteps = ref['snaps'][:, _t_field(w)]
    if name == 'pp':
        gate = ref['action'][:, -1]
        assert (gate == 0).any() and (gate == 1).any(), "the gate chain carries one value only"
    if name == 'tj_easy':
        assert (ref['alive'][1:] != ref['alive'][:-1]).any(), "no car's alive flag changes inside the window"
        assert (ref['alive'] == 0).any() and (ref['alive'] == 1).any()
    if name == 'pp_auto':
        assert ref['done'][:T - 1].any(), "no episode ends inside the window"
        assert (tsteps[1:] == 0).any(), "no env enters a step of the window at t == 0"


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_two_consecutive_wide_windows_write_the_bits_of_2T_per_step_calls(family):
    """What collection mode plays: the second window's step 0 is handed the first one's last masks and its slot T as slot 0, and
    reads them for every env that is mid-episode there (T = 5 slots over episodes of 2 steps: t = 1 at slot 5 unless a
    Predator-Prey episode ended by itself)."""
    w = _case('pp_auto', family)
    T = w['T']
    ref, win = _play_steps(w, family, 2 * T), _play_windows(w, family, 2)
    _compare(w, family, ref, win, "continue")
    tsteps = ref['snaps'][:, _t_field(w)]
    done = ref['done'].astype(bool)
    for k in (0, 1):
        assert done[k * T:(k + 1) * T - 1].any(0).all(), "window %d: an env does not restart strictly inside the window" % k
    assert (tsteps[1:T] == 0).any(), "no env enters a step of the first window at t == 0"
    assert (tsteps[T] != 0).any(), "every env enters the second window at t == 0: its step 0 would not read what it is handed"
    gate = ref['action'][T - 1, -1]
    assert (gate == 0).any() and (gate == 1).any(), "the gate handed to the second window carries one value only"


def _refusal_setup(family, hid=H, gate_split=True):
    w = dict(CASES['pp'], H=hid, E=5, T=2)
    env = _env(w, 3, 9)
    fam = _Lstm(w, env, 4, hid=hid, gate_split=gate_split) if family == 'lstm' else _Commnet(w, env, 4, family, hid=hid)
    b = _buffers(w, env, w['T'])
    if hid != H:                                                # (the records at the narrow widths' size: nothing may be written)
        R = w['E'] * w['N']
        for key, cols in (('hs', hid), ('cs', hid), ('gates', 4 * hid), ('inp', 2 * hid), ('h_fin', hid)):
            b[key] = np.full(b[key].shape[:1] + (R, cols), np.nan, np.float32)
    return w, env, fam, b


@pytest.mark.parametrize("what", ["hid64", "hid128", "size", "plain_tag", "obs", "no_split", "armed_hidden", "armed_record"])
@pytest.mark.parametrize("family", ["lstm", "tanh"])
def test_wide_refusals_come_before_any_launch(family, what):
    from ic3net_amd import _lib as binding
    hid = 64 if what == "hid64" else 128 if what == "hid128" else H
    w, env, fam, b = _refusal_setup(family, hid=hid, gate_split=not (family == 'lstm' and what == "no_split"))
    lib = env.lib
    before = {k: v.copy() for k, v in b.items()}
    state = env.raw_state()
    T = w['T']
    win = fam.struct(env, b, T) if not (family == 'tanh' and what == "no_split") else fam.struct(env, b, T, split=False)
    want = -22
    scratch = np.full((w['E'] * w['N'], 4 * hid), np.nan, np.float32)
    if what in ("hid64", "hid128", "no_split"):
        want = -38
    elif what == "size":
        win.struct_size = C.sizeof(win) + 8
    elif what == "plain_tag":
        win.struct_size = C.sizeof(binding.Policy)               # a plain ic3_policy that carries the value 6 / 7
    elif what == "armed_hidden":
        check(lib.ic3_env_set_hidden_out(env._h, p(scratch), p(scratch[:, hid:])))
    elif what == "armed_record":
        check(lib.ic3_env_set_record_out(env._h, p(scratch), None))
    obs = np.full((w['E'], w['N'], env.obs_dim), np.nan, np.float32) if what == "obs" else None
    _, comm_in = _masks0(w)
    rc = fam.window(env, b, T, None, comm_in, win=win, obs=obs)
    msg = lib.ic3_last_error().decode()
    assert rc == want, (what, rc, msg)
    tag = "ic3_policy_window" if family == 'lstm' else "ic3_commnet_window"
    assert msg.startswith("ic3_policy_step (%s, wide)" % tag), msg
    if what in ("hid64", "hid128"):
        narrow = "IC3_POLICY_WINDOW" if family == 'lstm' else "IC3_COMMNET_WINDOW"
        assert msg.count(narrow) > msg.count(narrow + "_WIDE"), "the message does not name the narrow tag: " + msg
    assert obs is None or np.isnan(obs).all()
    for key in COMMON + ALL_RECORDS:
        np.testing.assert_array_equal(b[key], before[key], err_msg=key)
    np.testing.assert_array_equal(env.raw_state(), state)
    assert np.isnan(scratch).all()
    if what.startswith("armed"):
        check(fam.window(env, b, T, None, comm_in))             # disarmed: the next call passes and writes its own record
        assert np.isfinite(b['hs'][1:]).all() and np.isfinite(b['out']).all() and np.isnan(scratch).all()
    env.close()

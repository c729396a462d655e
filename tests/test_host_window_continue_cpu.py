"""CPU: a window that CONTINUES running streams — `ic3_policy_step` on the three window descriptors (`ic3_policy_window`, the same tagged
`IC3_POLICY_WINDOW_PASSES`, `ic3_commnet_window` with and without the tanh recurrence) on an auto-reset handle, on the host build
(tests/host: the .hip sources unmodified behind the C ABI, `device = -1`), against per-step calls of the same library.

What the Trainer's collection mode plays: TWO consecutive windows of T = 8 slots over streams of 5-step episodes
(ic3_env_set_auto_reset(h, 5)).  Every env restarts strictly inside each window — at slot 4 of the first, at slots 1 and 6 of the
second (earlier where a Predator-Prey episode ends by itself) — and enters the second window mid-episode: its step 0 is handed the
first window's last alive slice / last-head draws and the first window's slot T as its slot 0, and reads them for every env whose
t != 0.  A twin handle from the same seed plays 2T per-step calls the way the header prescribes (ic3_env_snapshot in front of every
step, ic3_env_set_hidden_out to the next slot, the masks of step t - 1).  Everything written must be the SAME BITS: the (h, c) record,
out, action, reward, done, alive, is_completed, the snapshots, gates / inp or h_fin where recorded, and the state the handle is left in."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostPolicy, check, p
from test_host_commnet_window_cpu import make_weights
from test_host_policy_step_cpu import make_params
from test_host_policy_window_cpu import _env

T, E, EPISODE = 8, 12, 5

CASES = {
    # the gate chain: the last head's draws of step t - 1 are step t's gate (IC3_WINDOW_COMM_LAST_HEAD)
    'pp': dict(env='pp', N=3, dim=5, vision=0, H=64, heads=[5, 2], hard_attn=True, E=E, T=T, auto=EPISODE),
    # cars enter and leave: the alive slice of step t - 1 is step t's mask (IC3_WINDOW_ALIVE_PREV); a gate of ones (IC3_WINDOW_COMM_ONES)
    'tj_easy': dict(env='tj', N=5, dim=6, vision=1, difficulty='easy', H=128, heads=[2, 2], hard_attn=False, ones=True, rate=0.3, E=E,
                    T=T, auto=EPISODE),
}
# what each family records beside out / action / reward / done / alive / is_completed / snaps
FAMILIES = {'lstm': ('hs', 'cs', 'gates', 'inp'), 'lstm_p2': ('hs', 'cs'), 'commnet': ('h_fin',), 'tanh': ('hs', 'h_fin')}
COMMON = ('out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps')


def _buffers(w, env, n):
    """Sentinel-filled outputs of n slots; slot 0 of the state records holds noise an auto-reset handle must read as zero at t == 0."""
    N, H = w['N'], w['H']
    R, OT, nh = E * N, sum(w['heads']) + 1, len(w['heads'])
    f = lambda *s: np.full(s, np.nan, np.float32)
    i = lambda *s: np.full(s, -7, np.int32)
    b = dict(hs=f(n + 1, R, H), cs=f(n + 1, R, H), gates=f(n, R, 4 * H), inp=f(n, R, 2 * H), h_fin=f(n, R, H), out=f(n, R, OT),
             action=i(n, nh, R), reward=f(n, E, N), done=i(n, E), alive=i(n, E, N), comp=i(n, E, N), snaps=i(n, env.dims.state_words))
    rng = np.random.default_rng(11)
    b['hs'][0] = (rng.standard_normal((R, H)) * 0.3).astype(np.float32)
    b['cs'][0] = (rng.standard_normal((R, H)) * 0.3).astype(np.float32)
    return b


def _masks0(w):
    """(alive_in, comm_in) of the step that starts the streams: info is empty; the gate starts at 0 (hard_attn) or is ones."""
    return None, (np.zeros((E, w['N']), np.int32) if w['hard_attn'] else np.ones((E, w['N']), np.int32))


def _masks_after(w, b, t):
    """(alive_in, comm_in) the Trainer hands over behind step t."""
    return (b['alive'][t] if w['env'] == 'tj' else None,
            b['action'][t, len(w['heads']) - 1].reshape(E, w['N']) if w['hard_attn'] else np.ones((E, w['N']), np.int32))


def _modes(w):
    from ic3net_amd import _lib as binding
    W = binding.PolicyWindow
    return (W.ALIVE_PREV if w['env'] == 'tj' else W.ALIVE_ALL, W.COMM_LAST_HEAD if w['hard_attn'] else W.COMM_ONES)


class _Lstm(object):
    """ic3_policy_step / ic3_policy_window; passes == 2: the in-launch pass loop / IC3_POLICY_WINDOW_PASSES (no gate record)."""

    def __init__(self, w, env, seed, passes):
        self.w, self.passes = w, passes
        P = make_params(env.obs_dim, w['H'], w['heads'], seed=seed, comm_passes=passes)
        self.pol = HostPolicy(env, P, w['H'], w['heads'], gate_split=True, passes=passes)

    def step(self, env, b, t, alive_in, comm_in):
        check(env.lib.ic3_env_set_hidden_out(env._h, p(b['hs'][t + 1]), p(b['cs'][t + 1])))
        if self.passes == 1:
            check(env.lib.ic3_env_set_record_out(env._h, p(b['gates'][t]), p(b['inp'][t])))
        check(env.lib.ic3_policy_step(env._h, C.byref(self.pol.struct), p(b['hs'][t]), p(b['cs'][t]), p(alive_in), p(comm_in),
                                      p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]), p(b['done'][t]), p(b['alive'][t]),
                                      p(b['comp'][t]), None))

    def window(self, env, b, alive_in, comm_in):
        from ic3net_amd import _lib as binding
        win = binding.PolicyWindow()
        C.memmove(C.addressof(win), C.addressof(self.pol.struct), C.sizeof(self.pol.struct))
        win.struct_size = C.sizeof(win)
        win.inner_pass = win.WINDOW if self.passes == 1 else win.WINDOW_PASSES
        win.T = T
        win.alive_mode, win.comm_mode = _modes(self.w)
        if self.passes == 1:
            win.gates, win.inp = b['gates'].ctypes.data, b['inp'].ctypes.data
        win.snaps, win.snap_words = b['snaps'].ctypes.data, env.dims.state_words
        check(env.lib.ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(binding.Policy)), p(b['hs']), p(b['cs']), p(alive_in),
                                      p(comm_in), p(b['out']), p(b['action']), None, p(b['reward']), p(b['done']), p(b['alive']),
                                      p(b['comp']), None))


class _Commnet(object):
    """ic3_commnet_step / ic3_commnet_window: two passes with the communication block on and an h_fin record (recurrence 0), or the
    tanh recurrence — one pass, the block off — through the h record (recurrence 1; its h_fin record = the h slots behind)."""

    def __init__(self, w, env, seed, tanh):
        self.w, self.tanh = dict(w, passes=1 if tanh else 2), tanh
        self.cw = make_weights(env, self.w, seed)
        self.sizes = np.array(w['heads'], np.int32)

    def step(self, env, b, t, alive_in, comm_in):
        w, cw = self.w, self.cw
        h_in, h_out = (p(b['hs'][t]), p(b['hs'][t + 1])) if self.tanh else (None, p(b['h_fin'][t]))
        check(env.lib.ic3_commnet_step(env._h, p(cw['wt']), p(cw['enc_bias']), None, w['H'], w['passes'], p(cw['wp']), p(cw['wp3']),
                                       p(cw['bias']), p(cw['head_w']), p(cw['head_b']), p(self.sizes), len(w['heads']), 1, int(self.tanh),
                                       p(alive_in), p(comm_in), h_in, h_out, p(b['out'][t]), p(b['action'][t]), None, p(b['reward'][t]),
                                       p(b['done'][t]), p(b['alive'][t]), p(b['comp'][t]), None))
        if self.tanh:                                              # (the per-step call has one h_out: the recurrence's next slot)
            b['h_fin'][t] = b['hs'][t + 1]

    def window(self, env, b, alive_in, comm_in):
        from ic3net_amd import _lib as binding
        w, cw = self.w, self.cw
        win = binding.CommnetWindow()
        win.inner_pass = win.WINDOW
        win.H, win.nheads, win.mode_avg, win.comm_zero, win.npasses = w['H'], len(w['heads']), 1, int(self.tanh), w['passes']
        for k, A in enumerate(w['heads']):
            win.head_sizes[k] = A
        win.enc_wt, win.enc_bias = cw['wt'].ctypes.data, cw['enc_bias'].ctypes.data
        win.head_w, win.head_b = cw['head_w'].ctypes.data, cw['head_b'].ctypes.data
        win.T, win.recurrence = T, int(self.tanh)
        win.alive_mode, win.comm_mode = _modes(w)
        win.wp, win.bias, win.wp3 = cw['wp'].ctypes.data, cw['bias'].ctypes.data, cw['wp3'].ctypes.data
        win.h_fin = b['h_fin'].ctypes.data
        win.snaps, win.snap_words = b['snaps'].ctypes.data, env.dims.state_words
        check(env.lib.ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(binding.Policy)), p(b['hs']) if self.tanh else None, None,
                                      p(alive_in), p(comm_in), p(b['out']), p(b['action']), None, p(b['reward']), p(b['done']),
                                      p(b['alive']), p(b['comp']), None))


def _family(w, env, family, seed):
    if family in ('lstm', 'lstm_p2'):
        return _Lstm(w, env, seed, 2 if family == 'lstm_p2' else 1)
    return _Commnet(w, env, seed, family == 'tanh')


def _play_steps(w, family, seed=7, offset=40):
    """2T per-step calls on one handle, their slots in one record of 2T (+ 1) slots."""
    env = _env(w, seed, offset)
    fam = _family(w, env, family, seed + 1)
    b = _buffers(w, env, 2 * T)
    alive_in, comm_in = _masks0(w)
    for t in range(2 * T):
        b['snaps'][t] = env.snapshot()
        fam.step(env, b, t, alive_in, comm_in)
        alive_in, comm_in = _masks_after(w, b, t)
    b['state'] = env.raw_state()
    env.close()
    return b


def _play_windows(w, family, seed=7, offset=40):
    """Two window calls on one handle, each into a record of its own; the second continues the first.  Returns them joined to
    the shape of _play_steps' record."""
    env = _env(w, seed, offset)
    fam = _family(w, env, family, seed + 1)
    first, second = _buffers(w, env, T), _buffers(w, env, T)
    fam.window(env, first, *_masks0(w))
    second['hs'][0], second['cs'][0] = first['hs'][T], first['cs'][T]      # (NaN where the family keeps no such record)
    fam.window(env, second, *_masks_after(w, first, T - 1))
    b = {k: np.concatenate([first[k][:T], second[k]]) for k in first}
    b['state'] = env.raw_state()
    b['first'] = first
    env.close()
    return b


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_consecutive_windows_write_the_bits_of_2T_per_step_calls(name, family):
    w = CASES[name]
    ref, win = _play_steps(w, family), _play_windows(w, family)
    for key in COMMON + FAMILIES[family] + ('state',):
        np.testing.assert_array_equal(win[key], ref[key], err_msg="%s %s: %s" % (name, family, key))
    for key in set(sum(FAMILIES.values(), ())) - set(FAMILIES[family]) - {'hs', 'cs'}:
        assert np.isnan(win[key]).all() and np.isnan(ref[key]).all(), "%s: a record this family does not keep was written" % key
    for key in FAMILIES[family]:
        assert np.isfinite(ref[key][1:] if key in ('hs', 'cs') else ref[key][..., :w['H']]).all(), key
    assert np.isfinite(ref['out']).all() and (ref['action'] >= 0).all()
    np.testing.assert_array_equal(win['first']['hs'][T], win['hs'][T])
    # the conditions the test exists for, on the per-step side's draws
    env = _env(w, 7, 40)
    t_off, t_cnt = env._field('t')
    env.close()
    tsteps = ref['snaps'][:, t_off:t_off + t_cnt]
    done = ref['done'].astype(bool)
    for k in (0, 1):
        inside = done[k * T:(k + 1) * T - 1]
        assert inside.any(), "window %d: no env ends an episode before the window's last slot" % k
        assert inside.any(0).all(), "window %d: an env does not restart strictly inside the window" % k
    assert (tsteps[T] != 0).all(), "an env enters the second window at t == 0: its step 0 would not read what it is handed"
    first_end = lambda d: np.argmax(d, axis=0)
    assert (first_end(done[:T]) != first_end(done[T:])).all(), "an env restarts at the same slot in both windows"
    assert len({ref['snaps'][t].tobytes() for t in range(2 * T)}) == 2 * T, "two steps enter on the same state"
    if w['hard_attn']:
        gate = ref['action'][T - 1, -1]
        assert (gate == 0).any() and (gate == 1).any(), "the gate handed to the second window carries one value only"
    if w['env'] == 'tj':
        assert (ref['alive'][T - 1] == 0).any() and (ref['alive'][T - 1] == 1).any(), "the alive slice handed over is constant"


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_second_window_reads_what_it_is_handed(family):
    """The comparison above would pass on a kernel that ignored step 0's inputs only if the per-step side ignored them too; show
    that they matter: the second window from a zeroed slot 0 (recurrent families) or other masks (the gate chain) gives other rows."""
    w = CASES['pp']
    good = _play_windows(w, family)
    env = _env(w, 7, 40)
    fam = _family(w, env, family, 8)
    first, second = _buffers(w, env, T), _buffers(w, env, T)
    fam.window(env, first, *_masks0(w))
    second['hs'][0], second['cs'][0] = 0.0, 0.0
    fam.window(env, second, *_masks0(w))                           # zero gate, zero state: what a STARTING window is handed
    env.close()
    np.testing.assert_array_equal(first['out'], good['out'][:T])
    assert not np.array_equal(second['out'][0], good['out'][T])

"""GPU: a window that CONTINUES running streams — the cases of tests/test_host_window_continue_cpu.py on the device, BIT FOR BIT.

`ic3_policy_step` on an `ic3_policy_window` (one pass, and tagged IC3_POLICY_WINDOW_PASSES with two) and on an `ic3_commnet_window`
(recurrence 0 and 1) on an auto-reset handle of 5-step episodes: TWO consecutive windows of T = 8 slots, the second handed the
first's last alive slice / last-head draws and its slot T as slot 0, against 2T per-step launches on a twin handle (ic3_env_snapshot
in front of every step, ic3_env_set_hidden_out to the next slot, the masks of step t - 1).  Every env restarts strictly inside each
window, at another slot in the second than in the first, and enters the second window mid-episode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_commnet_step_window_gpu as cwin  # noqa: E402
import test_policy_window_gpu as pwin  # noqa: E402
import test_policy_window_passes_gpu as mwin  # noqa: E402

T, E, EPISODE = 8, 12, 5

CASES = {
    'pp': dict(kind='pp', env=dict(N=3, dim=5, vision=0, mode='mixed'), H=64, hard_attn=True, auto=EPISODE),
    'tj_easy': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=128,
                    hard_attn=False, ones=True, auto=EPISODE),
}
FAMILIES = {'lstm': ('hs', 'cs', 'gates', 'inp'), 'lstm_p2': ('hs', 'cs'), 'commnet': ('h_fin',), 'tanh': ('hs', 'h_fin')}
COMMON = ('out', 'action', 'reward', 'done', 'alive', 'comp', 'snaps', 'state')


class _Family(object):
    """One policy family on one handle: step(b, t, masks) = the per-step launch into slot t, window(b, masks) = T slots at once."""

    def __init__(self, w, family):
        self.w, self.family, self.lstm = w, family, family in ('lstm', 'lstm_p2')
        self.tanh, self.passes = family == 'tanh', 2 if family == 'lstm_p2' else 1
        if self.lstm:
            self.env, _, self.weights, self.heads = (pwin if family == 'lstm' else mwin)._setup(dict(w, passes=self.passes), E)
        else:       # (two heads for the gate of ones too, as on the host; one pass with the communication block off for the recurrence)
            self.env, self.weights, self.heads = cwin._setup(dict(w, hard_attn=True, passes=1 if self.tanh else 2), E)
        self.tj = w['kind'] == 'tj'
        self.comm_mode = 'last_head' if w['hard_attn'] else 'ones'

    def buffers(self, n):
        env, H = self.env, self.w['H']
        N, dev = env.nagents_env, env.device
        R, OT, nh = E * N, sum(self.heads) + 1, len(self.heads)
        f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
        i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
        b = dict(hs=f(n + 1, R, H), cs=f(n + 1, R, H), gates=f(n, R, 4 * H), inp=f(n, R, 2 * H), h_fin=f(n, R, H), out=f(n, R, OT),
                 action=i(n, nh, E, N), reward=f(n, E, N), done=i(n, E), alive=i(n, E, N), comp=i(n, E, N),
                 snaps=i(n, env.dims.state_words))
        g = torch.Generator(device='cpu').manual_seed(11)          # (an auto-reset handle reads slot 0 as zero at t == 0)
        b['hs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
        b['cs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
        return b

    def masks0(self):
        N, dev = self.env.nagents_env, self.env.device
        return None, (torch.zeros if self.w['hard_attn'] else torch.ones)((E, N), dtype=torch.int32, device=dev)

    def masks_after(self, b, t):
        N, dev = self.env.nagents_env, self.env.device
        return (b['alive'][t] if self.tj else None,
                b['action'][t, len(self.heads) - 1] if self.w['hard_attn'] else torch.ones((E, N), dtype=torch.int32, device=dev))

    def step(self, b, t, alive_in, comm_in):
        from ic3net_amd import ops
        env, H = self.env, self.w['H']
        env.snapshot(out=b['snaps'][t])
        if self.lstm:
            env.set_hidden_out(b['hs'][t + 1], b['cs'][t + 1])
            if self.passes == 1:
                env.set_record_out(b['gates'][t], b['inp'][t])
            ops.policy_step(env, self.weights, H, self.heads, True, False, b['hs'][t], b['cs'][t], alive_in, comm_in, b['out'][t],
                            b['action'][t], b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t], passes=self.passes)
        else:
            ops.commnet_step(env, self.weights, H, self.heads, True, self.tanh, alive_in, comm_in, b['out'][t], b['action'][t],
                             b['reward'][t], b['done'][t], b['alive'][t], b['comp'][t], h_in=b['hs'][t] if self.tanh else None,
                             h_out=b['hs'][t + 1] if self.tanh else b['h_fin'][t])
            if self.tanh:                                          # (the per-step call has one h_out: the recurrence's next slot)
                b['h_fin'][t].copy_(b['hs'][t + 1])

    def window(self, b, alive_in, comm_in):
        from ic3net_amd import ops
        env, H = self.env, self.w['H']
        if self.lstm:
            one = self.passes == 1
            ops.policy_step_window(env, self.weights, H, self.heads, True, False, T, b['hs'], b['cs'], alive_in, comm_in, b['out'],
                                   b['action'], b['reward'], b['done'], b['alive'], b['comp'], gates=b['gates'] if one else None,
                                   inp=b['inp'] if one else None, snaps=b['snaps'], alive_prev=self.tj, comm_mode=self.comm_mode,
                                   passes=self.passes)
        else:
            ops.commnet_step_window(env, self.weights, H, self.heads, True, self.tanh, T, alive_in, comm_in, b['out'], b['action'],
                                    b['reward'], b['done'], b['alive'], b['comp'], hs=b['hs'] if self.tanh else None, h_fin=b['h_fin'],
                                    snaps=b['snaps'], alive_prev=self.tj, comm_mode=self.comm_mode)

    def leave(self, b):
        torch.cuda.current_stream().synchronize()
        b['state'] = self.env.snapshot()
        return b


def _play_steps(w, family):
    fam = _Family(w, family)
    b = fam.buffers(2 * T)
    masks = fam.masks0()
    with torch.no_grad():
        for t in range(2 * T):
            fam.step(b, t, *masks)
            masks = fam.masks_after(b, t)
    return fam.leave(b)


def _play_windows(w, family):
    fam = _Family(w, family)
    first, second = fam.buffers(T), fam.buffers(T)
    with torch.no_grad():
        fam.window(first, *fam.masks0())
        second['hs'][0].copy_(first['hs'][T])                      # (NaN where the family keeps no such record)
        second['cs'][0].copy_(first['cs'][T])
        fam.window(second, *fam.masks_after(first, T - 1))
    b = {k: torch.cat([first[k][:T], second[k]]) for k in first}
    return fam.leave(b)


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_consecutive_windows_write_the_bits_of_2T_per_step_launches(name, family):
    w = CASES[name]
    ref, win = _play_steps(w, family), _play_windows(w, family)
    for key in COMMON + FAMILIES[family]:
        x, y = win[key].view(torch.int32), ref[key].view(torch.int32)     # bits (the untouched halves of inp hold NaN on both sides)
        assert torch.equal(x, y), "%s %s: %s differs in %d words" % (name, family, key, int((x != y).sum()))
    assert bool(torch.isfinite(ref['out']).all()) and bool((ref['action'] >= 0).all())
    for key in FAMILIES[family]:
        assert bool(torch.isfinite(ref[key][1:] if key in ('hs', 'cs') else ref[key][..., :w['H']]).all()), key
    # the conditions the test exists for, on the per-step side's draws
    done = ref['done'].to(torch.bool)
    for k in (0, 1):
        inside = done[k * T:(k + 1) * T - 1]
        assert bool(inside.any(0).all()), "window %d: an env does not restart strictly inside the window" % k
    first_end = lambda d: d.to(torch.int32).argmax(0)
    assert bool((first_end(done[:T]) != first_end(done[T:])).all()), "an env restarts at the same slot in both windows"
    assert not bool(done[T - 1].any()), "an env enters the second window at t == 0: its step 0 would not read what it is handed"

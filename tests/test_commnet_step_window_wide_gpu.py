"""GPU: `ic3_policy_step` on an `ic3_commnet_window` tagged IC3_COMMNET_WINDOW_WIDE — T steps of `ic3_commnet_step` at hid 256 in ONE
launch (commnet_forward_kernel<256, KIND, narrow | wide tile, false, 1>: one workgroup of 512 threads per CU) — against T per-step
launches of the same library on a twin handle, BIT FOR BIT: out, action, reward, done, alive, is_completed, all T snapshots, h slots
1 .. T of the tanh recurrence or the h_fin record, and the state the handle is left in.

The cases are those of tests/test_host_window_wide_cpu.py — the non-recurrent module with two passes, the IC baseline's stand-in
(narrow tile, h_fin), the tanh recurrence (hs) — plus what only the device has: more tiles than workgroup slots for both tiles (one
workgroup per CU at this width: a CU plays a second tile with its vector L1 warm), the window twice from the same state, the window
on the caller's non-default stream, two consecutive windows on an auto-reset handle, and the answers of the *_supported queries."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_commnet_step_window_gpu import _same, _setup  # noqa: E402

H = 256
_PP = dict(kind='pp', env=dict(N=3, dim=5, vision=1, mode='mixed'), H=H)
CASES = {
    # 21 envs per 64-row tile: one full and one ragged tile; the gate chain, two passes
    'pp_commnet_p2': dict(_PP, hard_attn=True, passes=2, E=23, T=3),
    # cars enter and leave inside the window; the IC baseline's stand-in (narrow tile) with its h_fin record
    'tj_easy_ic': dict(kind='tj', env=dict(N=5, dim=6, vision=1, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), H=H,
                       hard_attn=False, passes=1, ic=True, E=14, T=4),
    # the tanh recurrence on an auto-reset handle: episodes of 2 steps restart inside the window, their rows read as zero
    'pp_tanh_auto': dict(_PP, hard_attn=False, passes=1, tanh=True, auto=2, E=23, T=5),
    # the two-pass module on an auto-reset handle with the gate chain
    'pp_commnet_auto': dict(_PP, hard_attn=True, passes=2, auto=2, E=23, T=5),
}


def _play(w, windows, nwin=1):
    """windows False: nwin * T per-step launches; True: nwin consecutive window launches of T steps, each continuing the one before.
    One record of all slots either way."""
    from ic3net_amd import ops
    E, T = w['E'], w['T']
    env, cn, heads = _setup(w, E)
    N, dev = env.nagents_env, env.device
    R, OT, nh, n = E * N, sum(heads) + 1, len(heads), nwin * T
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(out=f(n, R, OT), action=i(n, nh, E, N), reward=f(n, E, N), done=i(n, E), alive=i(n, E, N), comp=i(n, E, N),
             snaps=i(n, env.dims.state_words), hs=f(n + 1, R, H), h_fin=f(n, R, H))
    b['hs'][0] = (torch.randn((R, H), generator=torch.Generator(device='cpu').manual_seed(11)) * 0.3).to(dev)
    tj, tanh, ic = w['kind'] == 'tj', bool(w.get('tanh')), bool(w.get('ic'))
    cz = tanh or ic
    alive_in = None
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else None
    after = lambda t: (b['alive'][t] if tj else None, b['action'][t, nh - 1] if w['hard_attn'] else None)
    with torch.no_grad():
        if windows:
            assert ops.commnet_step_window_supported(env, cn, H, wide=True)
            for k in range(nwin):
                s = slice(k * T, (k + 1) * T)
                ops.commnet_step_window(env, cn, H, heads, True, cz, T, alive_in, comm_in, b['out'][s], b['action'][s], b['reward'][s],
                                        b['done'][s], b['alive'][s], b['comp'][s], hs=b['hs'][k * T:(k + 1) * T + 1] if tanh else None,
                                        h_fin=b['h_fin'][s] if ic else None, snaps=b['snaps'][s], alive_prev=tj,
                                        comm_mode='last_head' if w['hard_attn'] else 'all', wide=True)
                alive_in, comm_in = after((k + 1) * T - 1)
        else:
            for t in range(n):
                env.snapshot(out=b['snaps'][t])
                ops.commnet_step(env, cn, H, heads, True, cz, alive_in, comm_in, b['out'][t], b['action'][t], b['reward'][t],
                                 b['done'][t], b['alive'][t], b['comp'][t], h_in=b['hs'][t] if tanh else None,
                                 h_out=b['hs'][t + 1] if tanh else b['h_fin'][t] if ic else None)
                alive_in, comm_in = after(t)
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    b['t_field'] = env.get_state()['t']
    return b


_REF = {}


def _ref(name, nwin=1):
    if (name, nwin) not in _REF:
        _REF[(name, nwin)] = _play(CASES[name], False, nwin)
    return _REF[(name, nwin)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_wide_window_launch_writes_the_bits_of_T_per_step_launches(name):
    w = CASES[name]
    ref, win = _ref(name), _play(w, True)
    _same(win, ref, name)
    T = w['T']
    assert bool(torch.isfinite(ref['out']).all()) and bool((ref['action'] >= 0).all())
    assert bool(torch.isfinite(ref['hs']).all()) == bool(w.get('tanh')) and bool(torch.isfinite(ref['h_fin']).all()) == bool(w.get('ic'))
    if w['hard_attn']:
        gate = ref['action'][:, -1]
        assert bool((gate == 0).any()) and bool((gate == 1).any()), "the gate chain carries one value only"
    if w['kind'] == 'tj':
        assert bool((ref['alive'][1:] != ref['alive'][:-1]).any()), "no car's alive flag changes inside the window"
    if w.get('auto'):
        assert bool(ref['done'][:T - 1].any()), "no episode ends inside the window"


@pytest.mark.parametrize("name", ['pp_commnet_auto', 'pp_tanh_auto'])
def test_two_consecutive_wide_windows_write_the_bits_of_2T_per_step_launches(name):
    w = CASES[name]
    T = w['T']
    ref, win = _ref(name, 2), _play(w, True, 2)
    _same(win, ref, "two windows, " + name)
    done = ref['done'].to(torch.bool)
    assert bool(done[:T - 1].any()) and bool(done[T:2 * T - 1].any()), "no episode ends inside one of the windows"


def _many_tiles(narrow):
    """More tiles than workgroup slots (ONE workgroup per CU at hid 256, either tile) + 64: N 10 -> 6 envs per tile."""
    key = 'many_narrow' if narrow else 'many_wide'
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    E = 6 * (cus + 64) + 3
    w = dict(kind='pp', env=dict(N=10, dim=5, vision=0, mode='mixed'), H=H, hard_attn=not narrow, passes=1, ic=narrow, E=E, T=4)
    if key not in _REF:
        _REF[key] = (_play(w, False), _play(w, True), w)
    return _REF[key]


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_more_tiles_than_workgroup_slots(narrow):
    ref, win, w = _many_tiles(narrow)
    _same(win, ref, "E = %d" % w['E'])


def test_the_window_twice_from_the_same_state_is_the_same_bits():
    _, win, w = _many_tiles(False)
    _same(_play(w, True), win, "second play, E = %d" % w['E'])


def test_the_window_on_the_callers_stream():
    w = CASES['tj_easy_ic']
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        win = _play(w, True)
    side.synchronize()
    _same(win, _ref('tj_easy_ic'), "side stream")


def test_supported_answers_and_refusals():
    from ic3net_amd import ops
    from ic3net_amd.comm import CommNetMLP
    w = CASES['pp_tanh_auto']
    for hid in (64, 128, 256):
        env, cn, heads = _setup(w, 5, H=hid)
        assert ops.commnet_step_window_supported(env, cn, hid, wide=True) == (hid == 256)
        assert ops.commnet_step_window_supported(env, cn, hid) == (hid != 256)          # the narrow tag's answers stay
    # hid 256 stays in `env, cn, heads`.  The narrow tag is still refused there, the wide one at another width too
    N, T, R = 3, 2, 15
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    args = lambda hid: (hid, heads, True, True, T, None, None, z(T, R, 6), z(T, 1, 5, N, dt=torch.int32), z(T, 5, N),
                        z(T, 5, dt=torch.int32), None, None)
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_commnet_window\)"):
        ops.commnet_step_window(env, cn, *args(256), hs=z(T + 1, R, H))
    with pytest.raises(AssertionError):
        ops.commnet_step_window(env, cn, *args(64), hs=z(T + 1, R, 64), wide=True)
    env.set_hidden_out(z(R, H), z(R, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_commnet_window, wide\)"):
        ops.commnet_step_window(env, cn, *args(256), hs=z(T + 1, R, H), wide=True)
    ops.commnet_step_window(env, cn, *args(256), hs=z(T + 1, R, H), wide=True)     # disarmed by the refused call
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_commnet_window, wide\)"):
        ops.commnet_step_window(env, dict(cn, wp3=None), *args(256), hs=z(T + 1, R, H), wide=True)
    # a zero-padded twin (hid 200 -> 256) keeps answering no
    torch.manual_seed(3)
    twin = CommNetMLP(argparse.Namespace(nagents=N, hid_size=200, comm_passes=2, recurrent=False, continuous=False, naction_heads=heads,
                                         comm_mask_zero=False, share_weights=False, comm_init='uniform', hard_attn=False,
                                         comm_mode='avg', rnn_type='MLP', init_std=0.2), env.obs_dim).cuda().float()
    twin.obs_encoder, twin.obs_table = env.encode, env.encode_table
    with torch.no_grad():
        assert ops.padded_hidden(200) == 256
        assert not twin.commnet_window_supported(env, wide=True) and not twin.commnet_window_supported(env)

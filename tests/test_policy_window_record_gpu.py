"""GPU: `ic3_policy_step` on an `ic3_policy_window_record` (tag IC3_POLICY_WINDOW_PASSES_RECORD) — the npasses window launch that also
stores every pass's activated gates, inp rows and entering (h, c): the MP + WIN + REC = 2 instantiations of csrc/policy_step.hip.  The
cases and the checks are those of tests/test_host_policy_window_record_cpu.py:

1. nothing else is disturbed — against one tag-5 launch on a twin handle, every key of tests/test_policy_window_passes_gpu.KEYS bit-equal;
2. the record bitwise against per-pass ic3_policy_step launches on a twin handle (h_pass / c_pass of every inner pass; the last pass's
   gates and inp rows through ic3_env_set_record_out; the h half of every inp_pass row keeps its sentinel);
3. every pass of the record against float64 (tests/window_record_util.py), within tests/window_record_bars.py;
4. refusals before any launch.

On the parent commit tag 9 is an unknown descriptor: every test here fails there."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_policy_window_passes_gpu import CASES, KEYS, _play, _same, _setup  # noqa: E402
import window_record_util as wr  # noqa: E402


def _buffers(w, env, heads):
    E, T, H = w['E'], w['T'], w['H']
    N, dev = env.nagents_env, env.device
    R, OT, nh = E * N, sum(heads) + 1, len(heads)
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    b = dict(hs=f(T + 1, R, H), cs=f(T + 1, R, H), out=f(T, R, OT), action=i(T, nh, E, N), reward=f(T, E, N), done=i(T, E),
             alive=i(T, E, N), comp=i(T, E, N), snaps=i(T, env.dims.state_words))
    g = torch.Generator(device='cpu').manual_seed(11)              # (the draws of test_policy_window_passes_gpu._play)
    b['hs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    b['cs'][0] = (torch.randn((R, H), generator=g) * 0.3).to(dev)
    return b


def _record(w, env, slots=None):
    P, T, R, H = slots or w['passes'], w['T'], w['E'] * env.nagents_env, w['H']
    f = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=env.device)
    return dict(gates=f(P, T, R, 4 * H), inp=f(P, T, R, 2 * H), h=f(P, T, R, H), c=f(P, T, R, H))


def _masks0(w, env):
    E, N, dev = w['E'], env.nagents_env, env.device
    comm_in = torch.zeros((E, N), dtype=torch.int32, device=dev) if w['hard_attn'] else \
        torch.ones((E, N), dtype=torch.int32, device=dev) if w.get('ones') else None
    return None, comm_in, 'last_head' if w['hard_attn'] else 'ones' if w.get('ones') else 'all'


def _play_record(w):
    from ic3net_amd import _lib, ops
    from ic3net_amd.ops import ptr, stream
    env, net, fc, heads = _setup(w, w['E'])
    b, rec = _buffers(w, env, heads), _record(w, env)
    alive_in, comm_in, comm_mode = _masks0(w, env)
    with torch.no_grad():
        assert ops.policy_step_window_supported(env, fc, w['H'], passes=w['passes'], record_passes=True)
        ops.policy_step_window(env, fc, w['H'], heads, True, False, w['T'], b['hs'], b['cs'], alive_in, comm_in, b['out'], b['action'],
                               b['reward'], b['done'], b['alive'], b['comp'], snaps=b['snaps'], alive_prev=w['kind'] == 'tj',
                               comm_mode=comm_mode, passes=w['passes'], record_passes=rec)
    torch.cuda.current_stream().synchronize()
    b['state'] = env.snapshot()
    obs = torch.empty((w['T'], w['E'], env.nagents_env, env.obs_dim), dtype=torch.float32, device=env.device)
    for t in range(w['T']):                                         # the dense rows of the state entering every step
        ops.check(_lib.lib().ic3_env_observe_at(env._h, ptr(b['snaps'][t]), ptr(obs[t]), stream()))
    torch.cuda.current_stream().synchronize()
    b['obs'] = obs
    off, cnt = C.c_int64(), C.c_int64()                           # the per-env step counter of every snapshot
    ops.check(_lib.lib().ic3_env_state_field(env._h, b"t", C.byref(off), C.byref(cnt)))
    assert cnt.value == w['E']
    b['t_enter'] = b['snaps'][:, off.value:off.value + cnt.value].cpu().numpy()
    return b, rec, net, heads


def _play_per_pass(w):
    """T steps of P per-pass launches each on a twin handle: what the record must hold where a launch leaves it behind."""
    from ic3net_amd import ops
    env, net, fc, heads = _setup(w, w['E'])
    n, T, H, nh = w['passes'], w['T'], w['H'], len(heads)
    b, rec = _buffers(w, env, heads), _record(w, env)
    alive_in, comm_in, _ = _masks0(w, env)
    with torch.no_grad():
        for t in range(T):
            h, c = b['hs'][t].clone(), b['cs'][t].clone()
            for i in range(n - 1):
                ops.policy_step_pass(env, fc, H, heads, True, False, h, c, alive_in, comm_in, i)
                rec['h'][i + 1, t].copy_(h)
                rec['c'][i + 1, t].copy_(c)
            env.set_record_out(rec['gates'][n - 1, t], rec['inp'][n - 1, t])
            ops.policy_step(env, fc, H, heads, True, False, h, c, alive_in, comm_in, b['out'][t], b['action'][t], b['reward'][t],
                            b['done'][t], b['alive'][t], b['comp'][t], pass_index=n - 1)
            b['hs'][t + 1].copy_(h)
            b['cs'][t + 1].copy_(c)
            if w['kind'] == 'tj':
                alive_in = b['alive'][t]
            if w['hard_attn']:
                comm_in = b['action'][t, nh - 1]
    torch.cuda.current_stream().synchronize()
    return b, rec


_PLAYED = {}


def _played(name):
    if name not in _PLAYED:
        _PLAYED[name] = _play_record(CASES[name])
    return _PLAYED[name]


def _bits(a, b, what):
    x, y = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(x, y), "%s differs in %d words" % (what, int((x != y).sum()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_recording_window_writes_the_bits_of_the_passes_window(name):
    w = CASES[name]
    b, rec, _, _ = _played(name)
    _same(b, _play(w, 'window'), name)
    assert bool(torch.isfinite(rec['gates']).all()) and bool(torch.isfinite(rec['inp'][..., :w['H']]).all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_record_is_what_the_per_pass_launches_leave_behind(name):
    w = CASES[name]
    n, H = w['passes'], w['H']
    b, rec, _, _ = _played(name)
    ref, want = _play_per_pass(w)
    for key in ('hs', 'cs', 'out', 'action', 'reward', 'done'):      # the twin did play the same window
        _bits(b[key], ref[key], "%s: %s" % (name, key))
    for i in range(1, n):
        _bits(rec['h'][i], want['h'][i], "%s: h_pass[%d]" % (name, i))
        _bits(rec['c'][i], want['c'][i], "%s: c_pass[%d]" % (name, i))
    assert bool(torch.isnan(rec['h'][0]).all()) and bool(torch.isnan(rec['c'][0]).all())
    _bits(rec['gates'][n - 1], want['gates'][n - 1], "%s: the last pass's gates" % name)
    _bits(rec['inp'][n - 1][..., :H], want['inp'][n - 1][..., :H], "%s: the last pass's inp" % name)
    assert bool(torch.isnan(rec['inp'][..., H:]).all()), "the h half of an inp_pass row was written"
    assert all(bool((rec['gates'][i] != rec['gates'][i + 1]).any()) for i in range(n - 1)), "two passes recorded the same gates"
    assert bool((rec['c'][1] != b['cs'][1:]).any()), "c_pass[1] is the step's final c"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_pass_of_the_record_against_float64(name):
    w = CASES[name]
    n, E, T, H = w['passes'], w['E'], w['T'], w['H']
    b, rec, net, heads = _played(name)
    N, nh = b['alive'].shape[2], len(heads)
    cpu = lambda x: x.detach().cpu().numpy()
    alive0, comm0, _ = _masks0(w, argparse_env(b, N))
    comm0 = None if comm0 is None else cpu(comm0)
    alive = [None] + [cpu(b['alive'][t - 1]) if w['kind'] == 'tj' else None for t in range(1, T)]
    gate = [comm0] + [cpu(b['action'][t - 1, nh - 1]) if w['hard_attn'] else comm0 for t in range(1, T)]
    fresh = (b['t_enter'] == 0) if w.get('auto') else None
    f = net.f_module
    ref = wr.reference_record(n, E, N, H, cpu(b['obs']).reshape(T, E * N, -1), cpu(b['hs']), cpu(b['cs']), cpu(net.encoder.weight),
                              cpu(net.encoder.bias), [cpu(net.C_modules[i].weight) for i in range(n)],
                              [cpu(net.C_modules[i].bias) for i in range(n)], cpu(f.weight_ih), cpu(f.weight_hh),
                              cpu(f.bias_ih).astype(np.float64) + cpu(f.bias_hh).astype(np.float64), alive, gate, fresh)
    if name == 'pp_auto_p2':
        assert fresh[1:].any(), "no env restarts inside the window"
    wr.check('gpu/' + name, wr.record_errors(n, H, {k: cpu(v) for k, v in rec.items()}, ref))


class argparse_env(object):
    """What _masks0 reads of an env, for a window that has been played already."""

    def __init__(self, b, N):
        self.nagents_env, self.device = N, b['hs'].device


def _refusal_args(w, env, heads, T=2):
    N, H, E = env.nagents_env, w['H'], 5
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=env.device)
    return lambda: (heads, True, False, T, z(T + 1, E * N, H), z(T + 1, E * N, H), None, None, z(T, E * N, sum(heads) + 1),
                    z(T, len(heads), E, N, dt=torch.int32), z(T, E, N), z(T, E, dt=torch.int32))


def test_refusals():
    from ic3net_amd import _lib, ops
    w = CASES['pp_p2']
    env, net, fc, heads = _setup(w, 5)
    H, T, R = 64, 2, 5 * env.nagents_env
    assert ops.policy_step_window_supported(env, fc, H, passes=2, record_passes=True)
    assert not ops.policy_step_window_supported(env, fc, H, passes=1, record_passes=True)
    assert not ops.policy_step_window_supported(env, fc, H, passes=5, record_passes=True)
    assert not ops.policy_step_window_supported(env, fc, 256, passes=2, record_passes=True)
    args = _refusal_args(w, env, heads, T)
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=env.device)
    rec = dict(gates=nan(2, T, R, 4 * H), inp=nan(2, T, R, 2 * H), h=nan(2, T, R, H), c=nan(2, T, R, H))
    untouched = lambda: all(bool(torch.isnan(v).all()) for v in rec.values())
    env.set_hidden_out(nan(R, H), nan(R, H))
    with pytest.raises(ValueError, match=r"^ic3_policy_step \(ic3_policy_window, passes record\)"):
        ops.policy_step_window(env, fc, H, *args(), passes=2, record_passes=rec)
    assert untouched()
    fc32 = dict(fc, ps_l_wp3=None)
    with pytest.raises(NotImplementedError, match=r"^ic3_policy_step \(ic3_policy_window, passes record\)"):
        ops.policy_step_window(env, fc32, H, *args(), passes=2, record_passes=rec)
    assert untouched()
    # the descriptor itself: tag 9 on the window's own size, and a non-NULL h_pass[0]
    pol = ops._policy_struct(fc, H, heads, True, False, passes=2)
    a = args()
    for what in ("size", "h_pass0"):
        win = _lib.PolicyWindowRecord()
        C.memmove(C.addressof(win), C.addressof(pol), C.sizeof(pol))
        win.struct_size = C.sizeof(_lib.PolicyWindow) if what == "size" else C.sizeof(win)
        win.inner_pass, win.T = win.WINDOW_PASSES_RECORD, T
        for i in range(2):
            win.gates_pass[i], win.inp_pass[i] = rec['gates'][i].data_ptr(), rec['inp'][i].data_ptr()
        win.h_pass[1], win.c_pass[1] = rec['h'][1].data_ptr(), rec['c'][1].data_ptr()
        if what == "h_pass0":
            win.h_pass[0] = rec['h'][0].data_ptr()
        rc = _lib.lib().ic3_policy_step(env._h, C.cast(C.byref(win), C.POINTER(_lib.Policy)), ops.ptr(a[4]), ops.ptr(a[5]), None, None,
                                        ops.ptr(a[8]), ops.ptr(a[9]), None, ops.ptr(a[10]), ops.ptr(a[11]), None, None, ops.stream())
        msg = _lib.lib().ic3_last_error().decode()
        assert rc == -22 and msg.startswith("ic3_policy_step (ic3_policy_window, passes record)"), (what, rc, msg)
        torch.cuda.current_stream().synchronize()
        assert untouched(), what
    ops.policy_step_window(env, fc, H, *args(), passes=2, record_passes=rec)      # and the call itself goes through
    torch.cuda.current_stream().synchronize()
    assert bool(torch.isfinite(rec['gates']).all()) and bool(torch.isfinite(rec['h'][1]).all())

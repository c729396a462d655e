"""CPU: `ic3_policy_step` on an `ic3_policy_window_record` (tag IC3_POLICY_WINDOW_PASSES_RECORD) — the npasses window launch that also
stores every pass's activated gates, inp rows and entering (h, c) — on the host build (tests/host: policy_step.hip unmodified behind
the C ABI, `device = -1`).  The cases are the four of tests/test_host_policy_window_passes_cpu.py.

1. Nothing else is disturbed: one tag-9 call against one tag-5 call on a twin handle, every key of that test's KEYS bit-equal.
2. The record, bitwise where an oracle exists: per-pass ic3_policy_step calls on a twin handle (pass_index = i, inner_pass = 1 for all
   passes but the last; DESIGN.md section 9 holds them bit-identical to the in-launch pass loop).  h_pass[i] / c_pass[i] are the h / c
   those calls leave behind pass i - 1; ic3_env_set_record_out armed in front of each step's LAST call gives the last pass's gates
   and inp rows; the h half of every inp_pass row keeps its sentinel.
3. The record, every pass, against float64 (tests/window_record_util.py), within tests/window_record_bars.py.
4. Refusals come before any launch (sentinel-filled outputs, the record arrays among them, stay untouched).

On the parent commit tag 9 is an unknown descriptor: every test here fails there."""
import ctypes as C

import numpy as np
import pytest

from host_abi_util import HostPolicy, check, p
from test_host_policy_step_cpu import make_params
from test_host_policy_window_cpu import _buffers, _call_window, _env, _masks0, _untouched
from test_host_policy_window_passes_cpu import CASES, KEYS, _params, _passes_struct, _play
import window_record_util as wr

PREFIX = "ic3_policy_step (ic3_policy_window, passes record)"


def _record_buffers(w, slots=None):
    """NaN-filled record arrays, (slots, T, R, .): slot i is pass i's."""
    P, T, R, H = slots or w['passes'], w['T'], w['E'] * w['N'], w['H']
    f = lambda *s: np.full(s, np.nan, np.float32)
    return dict(gates=f(P, T, R, 4 * H), inp=f(P, T, R, 2 * H), h=f(P, T, R, H), c=f(P, T, R, H))


def _record_struct(pol, T, b, w, snap_words, rec, npasses=None, size=None, tag=None):
    """The tag-9 descriptor: the passes window's struct (tag 5's, no gate record) followed by the passes' arrays."""
    from ic3net_amd import _lib as binding
    win = _passes_struct(pol, T, b, w, snap_words)
    r = binding.PolicyWindowRecord()
    C.memmove(C.addressof(r), C.addressof(win), C.sizeof(win))
    r.struct_size = C.sizeof(r) if size is None else size
    r.inner_pass = r.WINDOW_PASSES_RECORD if tag is None else tag
    for i in range(w['passes'] if npasses is None else npasses):
        r.gates_pass[i], r.inp_pass[i] = rec['gates'][i].ctypes.data, rec['inp'][i].ctypes.data
        if i >= 1:
            r.h_pass[i], r.c_pass[i] = rec['h'][i].ctypes.data, rec['c'][i].ctypes.data
    return r


def _play_record(w, seed=7, offset=40):
    env = _env(w, seed, offset)
    P = _params(w, env.obs_dim, seed + 1)
    pol = HostPolicy(env, P, w['H'], w['heads'], gate_split=True, passes=w['passes'])
    b, rec = _buffers(w, env), _record_buffers(w)
    alive_in, comm_in = _masks0(w)
    check(_call_window(env, _record_struct(pol, w['T'], b, w, env.dims.state_words, rec), b, alive_in, comm_in))
    b['state'] = env.raw_state()
    # the dense observation of the state entering every step, for the float64 encoder rows
    b['obs'] = np.stack([env.observe(b['snaps'][t]) for t in range(w['T'])])
    t_off, _ = env._field('t')
    b['t_enter'] = b['snaps'][:, t_off:t_off + w['E']].copy()
    env.close()
    return b, rec, P


def _play_per_pass(w, seed=7, offset=40):
    """T steps of P per-pass calls each on a twin handle; returns what the record must hold where a call leaves it behind."""
    env = _env(w, seed, offset)
    P = _params(w, env.obs_dim, seed + 1)
    n, T, H, nh = w['passes'], w['T'], w['H'], len(w['heads'])
    pols = [HostPolicy(env, P, H, w['heads'], gate_split=True, pass_index=i, inner=i + 1 < n) for i in range(n)]
    b, rec = _buffers(w, env), _record_buffers(w)
    alive_in, comm_in = _masks0(w)
    for t in range(T):
        h, c = b['hs'][t].copy(), b['cs'][t].copy()
        for i in range(n - 1):
            pols[i].inner_pass(env, h, c, alive_in, comm_in)
            rec['h'][i + 1, t], rec['c'][i + 1, t] = h, c
        check(env.lib.ic3_env_set_record_out(env._h, p(rec['gates'][n - 1, t]), p(rec['inp'][n - 1, t])))
        check(env.lib.ic3_policy_step(env._h, C.byref(pols[n - 1].struct), p(h), p(c), p(alive_in), p(comm_in), p(b['out'][t]),
                                      p(b['action'][t]), None, p(b['reward'][t]), p(b['done'][t]), p(b['alive'][t]), p(b['comp'][t]),
                                      None))
        b['hs'][t + 1], b['cs'][t + 1] = h, c
        if w['env'] == 'tj':
            alive_in = b['alive'][t]
        if w['hard_attn']:
            comm_in = b['action'][t, nh - 1]
    env.close()
    return b, rec


def _step_masks(w, b):
    """(alive, gate) of every step, T entries each, as the window derives them from step t - 1."""
    T, nh = w['T'], len(w['heads'])
    alive0, comm0 = _masks0(w)
    alive = [alive0] + [b['alive'][t - 1] if w['env'] == 'tj' else None for t in range(1, T)]
    gate = [comm0] + [b['action'][t - 1, nh - 1].reshape(w['E'], w['N']) if w['hard_attn'] else comm0 for t in range(1, T)]
    return alive, gate


@pytest.fixture(scope="module")
def played():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _play_record(CASES[name])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_recording_window_writes_the_bits_of_the_passes_window(name, played):
    w = CASES[name]
    b, rec, _ = played(name)
    ref = _play(w, 'window')
    for key in KEYS:
        np.testing.assert_array_equal(b[key], ref[key], err_msg="%s: %s" % (name, key))
    assert np.isnan(b['gates']).all() and np.isnan(b['inp']).all(), "window.gates / window.inp are not this form's record"
    assert np.isfinite(rec['gates']).all() and np.isfinite(rec['inp'][..., :w['H']]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_record_is_what_the_per_pass_calls_leave_behind(name, played):
    w = CASES[name]
    n, H = w['passes'], w['H']
    b, rec, _ = played(name)
    ref, want = _play_per_pass(w)
    for key in ('hs', 'cs', 'out', 'action', 'reward', 'done'):      # the twin did play the same window
        np.testing.assert_array_equal(b[key], ref[key], err_msg="%s: %s" % (name, key))
    for i in range(1, n):
        np.testing.assert_array_equal(rec['h'][i], want['h'][i], err_msg="%s: h_pass[%d]" % (name, i))
        np.testing.assert_array_equal(rec['c'][i], want['c'][i], err_msg="%s: c_pass[%d]" % (name, i))
    assert np.isnan(rec['h'][0]).all() and np.isnan(rec['c'][0]).all()
    np.testing.assert_array_equal(rec['gates'][n - 1], want['gates'][n - 1], err_msg="%s: the last pass's gates" % name)
    np.testing.assert_array_equal(rec['inp'][n - 1][..., :H], want['inp'][n - 1][..., :H], err_msg="%s: the last pass's inp" % name)
    assert np.isnan(rec['inp'][..., H:]).all(), "the h half of an inp_pass row was written"
    # the passes differ: the record is not one pass's values n times
    assert all((rec['gates'][i] != rec['gates'][i + 1]).any() and (rec['inp'][i][..., :H] != rec['inp'][i + 1][..., :H]).any()
               for i in range(n - 1))
    assert (rec['c'][1] != b['cs'][1:]).any(), "c_pass[1] is the step's final c"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_pass_of_the_record_against_float64(name, played):
    w = CASES[name]
    n, E, N, H = w['passes'], w['E'], w['N'], w['H']
    b, rec, P = played(name)
    alive, gate = _step_masks(w, b)
    fresh = (b['t_enter'] == 0) if w.get('auto') else None
    ref = wr.reference_record(n, E, N, H, b['obs'].reshape(w['T'], E * N, -1), b['hs'], b['cs'], P['encoder.weight'], P['encoder.bias'],
                              [P['C_modules.%d.weight' % i] for i in range(n)], [P['C_modules.%d.bias' % i] for i in range(n)],
                              P['f_module.weight_ih'], P['f_module.weight_hh'], P['f_module.bias_ih'] + P['f_module.bias_hh'],
                              alive, gate, fresh)
    if name == 'pp_auto_p2':
        assert fresh[1:].any(), "no env restarts inside the window"
    wr.check('host/' + name, wr.record_errors(n, H, rec, ref))


def _refusal_setup(H=64, passes=2):
    w = dict(CASES['pp_p2'], H=H, E=5, T=3, passes=passes)
    env = _env(w, 3, 9)
    P = make_params(env.obs_dim, H, w['heads'], seed=4, comm_passes=passes)
    pol = HostPolicy(env, P, H, w['heads'], gate_split=True, passes=passes)
    return w, env, pol, _buffers(w, env), _record_buffers(w, slots=4)


@pytest.mark.parametrize("what", ["size", "plain", "forward", "missing_gates", "missing_inp", "missing_h", "h_pass0", "c_pass0",
                                  "window_gates", "hid256", "npasses1", "npasses5", "pass_index", "armed_hidden", "armed_record",
                                  "armed_events"])
def test_refusals_come_before_any_launch(what):
    from ic3net_amd import _lib as binding
    w, env, pol, b, rec = _refusal_setup(H=256 if what == "hid256" else 64, passes=4 if what == "npasses5" else 2)
    lib = env.lib
    before = {k: v.copy() for k, v in b.items()}
    before['state'] = env.raw_state()
    rec_before = {k: v.copy() for k, v in rec.items()}
    _, comm_in = _masks0(w)
    win = _record_struct(pol, w['T'], b, w, env.dims.state_words, rec, npasses=4)
    want = -22
    if what == "size":
        win.struct_size = C.sizeof(binding.PolicyWindow)         # tag 9 on the window's own size
        rc = _call_window(env, win, b, None, comm_in)
    elif what == "plain":                                       # a plain ic3_policy that carries the value 9
        pol.struct.inner_pass = binding.PolicyWindowRecord.WINDOW_PASSES_RECORD
        rc = lib.ic3_policy_step(env._h, C.byref(pol.struct), p(b['hs']), p(b['cs']), None, p(comm_in), p(b['out']), p(b['action']),
                                 None, p(b['reward']), p(b['done']), p(b['alive']), p(b['comp']), None)
    elif what == "forward":
        enc = np.zeros((w['E'] * w['N'], w['H']), np.float32)
        rc = lib.ic3_policy_forward(C.cast(C.byref(win), C.POINTER(binding.Policy)), p(enc), w['E'], w['N'], p(b['hs']), p(b['cs']),
                                    None, p(comm_in), p(b['out']), None)
    elif what in ("missing_gates", "missing_inp", "missing_h", "h_pass0", "c_pass0", "window_gates"):
        if what == "missing_gates":
            win.gates_pass[1] = None
        elif what == "missing_inp":
            win.inp_pass[0] = None
        elif what == "missing_h":
            win.h_pass[1] = None
        elif what == "h_pass0":
            win.h_pass[0] = rec['h'][0].ctypes.data
        elif what == "c_pass0":
            win.c_pass[0] = rec['c'][0].ctypes.data
        else:
            win.gates, win.inp = b['gates'].ctypes.data, b['inp'].ctypes.data
        rc = _call_window(env, win, b, None, comm_in)
    elif what in ("hid256", "npasses1", "npasses5", "pass_index"):
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
        if what == "armed_events":
            for e in ev:
                check(lib.ic3_event_destroy(e))
    msg = lib.ic3_last_error().decode()
    assert rc == want, (what, rc, msg)
    if what != "forward":
        assert msg.startswith(PREFIX), msg
    if what == "hid256":
        assert "256" in msg, msg
    _untouched(env, b, before)
    for k in rec:
        np.testing.assert_array_equal(rec[k], rec_before[k], err_msg=k)
    env.close()


def test_the_struct_is_the_header_s():
    """PolicyWindowRecord is ic3_policy_window followed by four arrays of four pointers (include/ic3_rollout.h)."""
    from ic3net_amd import _lib as binding
    assert C.sizeof(binding.PolicyWindowRecord) == C.sizeof(binding.PolicyWindow) + 16 * C.sizeof(C.c_void_p)
    assert binding.PolicyWindowRecord.gates_pass.offset == C.sizeof(binding.PolicyWindow)

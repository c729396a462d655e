"""CPU: the two calls behind the window backward of comm_passes > 1 policies — ic3_policy_forward as a recording inner pass (on an
ic3_policy_record) and ic3_bptt_backward on an ic3_bptt_passes descriptor (the window's backward as one host call) — on the host build of the product's own sources
(tests/host/libic3rollout_host.so) against the float64 multi-pass window of tests/bptt_passes_ref.py.

A window is built the way bptt._backward_window_multipass builds a chunk: one encoder launch per snapshot into a ring (encoder.bias +
C_0.bias), pass i as ONE recording launch over the T x E stacked envs from slot i of the (h, c) ring into slot i + 1 (C_i.bias -
C_0.bias added in the launch), then the backward call in place on those records and ic3_lstm_weight_grad_wide over the P x T x R rows."""
import ctypes as C

import numpy as np
import pytest

import bptt_passes_ref as ref
from host_abi_util import HostEnv, HostPolicy, check, host_lib, p
from test_host_policy_step_cpu import make_params

HEADS = [5, 2]
OT = sum(HEADS) + 1

CASES = {
    'h64-n3-E5-T3-P2-gap2': dict(env=lambda: HostEnv.pp(3, 6, 1, 'mixed', 5, seed=3), H=64, T=3, P=2, gap=2, alive='first_null'),
    'h64-n5-E3-T2-P3-share-comm-zero': dict(env=lambda: HostEnv.tj(5, 6, 1, 'easy', 3, seed=3, add_rate_min=0.6, add_rate_max=0.6),
                                            H=64, T=2, P=3, share=True, comm_zero=True, alive='all'),
    'h128-n10-E2-T2-P2-one-tile': dict(env=lambda: HostEnv.pp(10, 8, 1, 'mixed', 2, seed=3), H=128, T=2, P=2),
}


def xh_width(H):
    return H if H == 256 else 2 * H


def forward_record(pol, enc, enc_add, E, N, h_in, c_in, h_out, c_out, alive, gate, gates, inp):
    """ic3_policy_forward on an ic3_policy_record made of the policy's struct (size_off: a wrong struct_size) and these operands"""
    from ic3net_amd import _lib as binding
    rec = binding.PolicyRecord()
    C.memmove(C.addressof(rec), C.addressof(pol.struct), C.sizeof(pol.struct))
    rec.struct_size, rec.inner_pass = C.sizeof(rec) - getattr(pol, 'size_off', 0), rec.RECORD_PASS
    rec.enc_add, rec.h_out, rec.c_out, rec.gates, rec.inp = [None if a is None else a.ctypes.data for a in (enc_add, h_out, c_out, gates, inp)]
    return host_lib().ic3_policy_forward(C.cast(C.byref(rec), C.POINTER(binding.Policy)), p(enc), E, N, p(h_in), p(c_in), p(alive), p(gate),
                                         None, None)


def passes_backward(lib, env, b):
    """ic3_bptt_backward handed the ic3_bptt_passes descriptor (its magic says which one it is)"""
    return lib.ic3_bptt_backward(env._h, C.byref(b), None)


class Window(object):
    """Snapshots, parameters, masks and the forward records of one case; everything the backward call reads or writes."""

    def __init__(self, name, cfg):
        from test_host_abi_cpu import _play
        lib = host_lib()
        self.env = env = cfg['env']()
        self.T, self.H, self.P = T, H, P = cfg['T'], cfg['H'], cfg['P']
        self.E, self.N = E, N = env.E, env.N
        self.R = R = E * N
        self.comm_zero, self.avg = cfg.get('comm_zero', False), cfg.get('avg', True)
        rng = np.random.default_rng(sum(map(ord, name)))
        self.params = P64 = make_params(env.obs_dim, H, HEADS, seed=11, comm_passes=P)
        if cfg.get('share'):
            for i in range(1, P):
                P64['C_modules.%d.weight' % i], P64['C_modules.%d.bias' % i] = P64['C_modules.0.weight'], P64['C_modules.0.bias']
        self.pols = [HostPolicy(None, P64, H, HEADS, mode_avg=self.avg, comm_zero=self.comm_zero, gate_split=True, use_table=False,
                                pass_index=i, inner=True) for i in range(P)]
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        self.adds = [None] + [f32(P64['C_modules.%d.bias' % i] - P64['C_modules.0.bias']) for i in range(1, P)]
        snaps, obs, enc = [], [], []
        for t in range(T):
            _play(env, 2 + t, 70 + t)
            snaps.append(env.snapshot())
            obs.append(env.observe().reshape(R, env.obs_dim).astype(np.float64))
            enc.append(env.encode(self.pols[0].wt, self.pols[0].enc_bias, snap=snaps[-1]).reshape(R, H))
        self.snaps, self.obs = np.ascontiguousarray(np.stack(snaps)), obs
        self.enc = np.ascontiguousarray(np.stack(enc))                                      # (T, R, H): the encoder ring
        mask = lambda q: np.ascontiguousarray(rng.random((E, N)) < q, np.int32)
        am = cfg.get('alive', 'none')
        self.alive = None if am == 'none' else [None if (am == 'first_null' and t == 0) else mask(0.8) for t in range(T)]
        self.gate = [mask(0.6) for t in range(T)]
        # stacked masks of the T x E envs of a window-wide launch (a step without an alive mask: ones)
        self.alive_st = None if self.alive is None else np.ascontiguousarray(
            np.stack([np.ones((E, N), np.int32) if m is None else m for m in self.alive]))
        self.gate_st = np.ascontiguousarray(np.stack(self.gate))
        self.h0 = f32(np.tanh(rng.standard_normal((R, H))))
        self.c0 = f32(rng.standard_normal((R, H)))
        self.lib = lib

    def step_by_step(self):
        """The window played step by step, one recording launch per (step, pass) over E envs: the (h, c) entering every step."""
        T, P, R, H, E, N = self.T, self.P, self.R, self.H, self.E, self.N
        hs0, cs0 = np.zeros((T + 1, R, H), np.float32), np.zeros((T + 1, R, H), np.float32)
        hs0[0], cs0[0] = self.h0, self.c0
        rec = dict(gates=np.zeros((P, T, R, 4 * H), np.float32), h=np.zeros((P, T, R, H), np.float32), c=np.zeros((P, T, R, H), np.float32))
        for t in range(T):
            h, c = hs0[t].copy(), cs0[t].copy()
            for i in range(P):
                inp = np.full((R, xh_width(H)), np.nan, np.float32)
                check(forward_record(self.pols[i], self.enc[t], self.adds[i], E, N, h, c, h, c,        # (in place: allowed)
                                     None if self.alive is None else self.alive[t], self.gate[t], rec['gates'][i, t], inp))
                rec['h'][i, t], rec['c'][i, t] = h, c
            hs0[t + 1], cs0[t + 1] = h, c
        return hs0, cs0, rec

    def window_wide(self, hs0, cs0):
        """Pass i as ONE launch over the T x E stacked envs: slot i -> slot i + 1; NaN-filled outputs."""
        T, P, R, H, E, N = self.T, self.P, self.R, self.H, self.E, self.N
        nan = lambda *s: np.full(s, np.nan, np.float32)
        self.hsl, self.csl = nan(P + 1, T * R, H), nan(P + 1, T * R, H)
        self.hsl[0], self.csl[0] = hs0[:T].reshape(T * R, H), cs0[:T].reshape(T * R, H)
        self.gates, self.inp = nan(P, T * R, 4 * H), nan(P, T * R, xh_width(H))
        enc = self.enc.reshape(T * R, H)
        for i in range(P):
            h_in, c_in = self.hsl[i].copy(), self.csl[i].copy()
            check(forward_record(self.pols[i], enc, self.adds[i], T * E, N, self.hsl[i], self.csl[i], self.hsl[i + 1], self.csl[i + 1],
                                 self.alive_st, self.gate_st, self.gates[i], self.inp[i]))
            np.testing.assert_array_equal(self.hsl[i], h_in)      # the inputs keep their bits
            np.testing.assert_array_equal(self.csl[i], c_in)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_record_and_passes_backward_against_float64(name):
    """Forward: the stacked launches give the bits of the step-by-step ones (gates, h, c of every (step, pass)); gates, inp and the
    state every pass leaves against the float64 forward chained from the same (h0, c0); the h half of the 2H-wide inp rows untouched.
    Backward, on those records: dgates of every (t, i), the dxh rings, dh / dc leaving the window, EVERY row of each pass's bias
    partials, each pass's dcw sum, the encoder's dWt / db through the window finish, and dW of ic3_lstm_weight_grad_wide over the
    P x T x R rows — each against the float64 window backward at its bar (bptt_passes_ref.check)."""
    from ic3net_amd import _lib as binding
    cfg = CASES[name]
    win = Window(name, cfg)
    lib, env = win.lib, win.env
    T, P, R, H, E, N = win.T, win.P, win.R, win.H, win.E, win.N
    gap = cfg.get('gap', 0)
    hs0, cs0, rec = win.step_by_step()
    win.window_wide(hs0, cs0)
    for i in range(P):
        np.testing.assert_array_equal(win.gates[i].reshape(T, R, 4 * H), rec['gates'][i])
        np.testing.assert_array_equal(win.hsl[i + 1].reshape(T, R, H), rec['h'][i])
        np.testing.assert_array_equal(win.csl[i + 1].reshape(T, R, H), rec['c'][i])
    if H != 256:
        assert np.isnan(win.inp[:, :, H:]).all()
    P64 = win.params
    x = np.stack([o @ P64['encoder.weight'].T + P64['encoder.bias'] for o in win.obs])
    fwd = ref.window_forward(x, win.h0, win.c0, [P64['C_modules.%d.weight' % i] for i in range(P)],
                             [P64['C_modules.%d.bias' % i] for i in range(P)], P64['f_module.weight_ih'], P64['f_module.weight_hh'],
                             P64['f_module.bias_ih'] + P64['f_module.bias_hh'], E, N, alive=win.alive, gate=win.gate, mode_avg=win.avg,
                             comm_zero=win.comm_zero)
    r4 = lambda a, w: a.reshape(P, T, R, w)
    errs = dict(fwd_gates=ref.rel_err(r4(win.gates, 4 * H), fwd['gates']), fwd_inp=ref.rel_err(r4(win.inp[:, :, :H], H), fwd['inp']),
                fwd_h=ref.rel_err(win.hsl[1:].reshape(P, T, R, H)[:-1], fwd['hs'][1:]),
                fwd_c=ref.rel_err(win.csl[1:].reshape(P, T, R, H)[:-1], fwd['cs'][1:]))
    h_end = np.concatenate([fwd['hs'][0, 1:], fwd['h'][None]])   # what the last pass of every step leaves
    c_end = np.concatenate([fwd['cs'][0, 1:], fwd['c'][None]])
    errs['fwd_h'] = max(errs['fwd_h'], ref.rel_err(win.hsl[P].reshape(T, R, H), h_end))
    errs['fwd_c'] = max(errs['fwd_c'], ref.rel_err(win.csl[P].reshape(T, R, H), c_end))

    # ---- the backward on the records the launches left ----------------------------------------------------------------------------
    assert lib.ic3_bptt_backward_supported(env._h, H) == 1
    rng = np.random.default_rng(99)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    dhead, w_heads = f32(rng.standard_normal((T, R, OT))), win.pols[0].w_heads
    dh0, dc0 = f32(rng.standard_normal((R, H))), f32(rng.standard_normal((R, H)))
    cws = [win.pols[i].c_w for i in range(P)]
    want = ref.window_backward(r4(win.gates, 4 * H), win.hsl[:P].reshape(P, T, R, H), win.csl[:P].reshape(P, T, R, H), dhead, w_heads,
                               win.pols[0].w_ih, win.pols[0].w_hh, dh0, dc0, E, N, c_weights=cws, alive=win.alive, gate=win.gate,
                               detach_gap=gap, mode_avg=win.avg, comm_zero=win.comm_zero, obs=win.obs, inp=r4(win.inp[:, :, :H], H))
    dgates, dh, dc = win.gates.copy(), dh0.copy(), dc0.copy()
    dxh = np.full((P, T, R, 2 * H), np.nan, np.float32)
    tiles, slots = (R + 63) // 64, lib.ic3_comm_backward_partials(E, N)
    bias0, dcw0 = f32(rng.standard_normal((P, tiles, 4 * H))), f32(rng.standard_normal((P, slots, H, H)))
    bias, dcw = bias0.copy(), dcw0.copy()
    wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
    check(lib.ic3_policy_pack_split_bwd(p(win.pols[0].w_ih), p(win.pols[0].w_hh), p(wb3), H, None))
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H))
    assert n > 0
    work = np.full((n,), np.nan, np.float32)
    arr = lambda xs: C.cast((C.c_void_p * len(xs))(*[None if a is None else a.ctypes.data for a in xs]), C.POINTER(C.c_void_p))
    b = binding.BpttPasses(T, E, N, H, OT, P, int(win.avg), int(win.comm_zero), gap, 1, 0)
    keep = dict(gates=arr([dgates[i] for i in range(P)]), hs=arr([win.hsl[i] for i in range(P)]), cs=arr([win.csl[i] for i in range(P)]),
                dxh=arr([dxh[i] for i in range(P)]), dbias_partials=arr([bias[i] for i in range(P)]),
                dcw_partials=arr([dcw[i] for i in range(P)]), c_weight=arr(cws), gate=arr(win.gate))
    if win.alive is not None:
        keep['alive'] = arr(win.alive)
    for k, v in keep.items():
        setattr(b, k, v)
    b.dhead, b.snaps, b.snap_words = dhead.ctypes.data, win.snaps.ctypes.data, win.snaps.shape[1]
    b.lstm_wp3_bwd, b.w_heads, b.dh, b.dc = wb3.ctypes.data, w_heads.ctypes.data, dh.ctypes.data, dc.ctypes.data
    b.dxh_step, b.enc_work = R * 2 * H, work.ctypes.data
    # refused before the first launch: a pass without its ring — the records keep their bits
    b.dxh = arr([dxh[0]] + [None] * (P - 1))
    assert passes_backward(lib, env, b) == -22 and b"pass 1" in lib.ic3_last_error()
    np.testing.assert_array_equal(dgates, win.gates)
    np.testing.assert_array_equal(dh, dh0)
    np.testing.assert_array_equal(bias, bias0)
    assert np.isnan(dxh).all()
    b.dxh = keep['dxh']
    check(passes_backward(lib, env, b))
    errs.update(dgates=ref.rel_err(r4(dgates, 4 * H), want['dgates']), dxh=ref.rel_err(dxh, want['dxh']), dh=ref.rel_err(dh, want['dh']),
                dc=ref.rel_err(dc, want['dc']), dbias_rows=ref.rel_err(bias, bias0.astype(np.float64) + want['dbias_rows']))
    if win.comm_zero:
        np.testing.assert_array_equal(dcw, dcw0)                 # (nothing of C is touched)
    else:
        errs['dcw'] = ref.rel_err(dcw.astype(np.float64).sum(1), dcw0.astype(np.float64).sum(1) + want['dcw'])
    # the C_i.bias gradient from the bias partials: (column sums of pass i's dgates) . W_ih
    dcb = (bias.astype(np.float64) - bias0).sum(1) @ win.pols[0].w_ih.astype(np.float64)
    errs['dcb'] = ref.rel_err(dcb, want['dcb'])
    dwt, db = np.full((env.obs_dim, H), np.nan, np.float32), np.full((H,), np.nan, np.float32)
    check(lib.ic3_env_encode_backward_window_finish(env._h, H, p(dwt), p(db), p(work), None))
    errs['enc_dwt'], errs['enc_db'] = ref.rel_err(dwt, want['enc_dwt']), ref.rel_err(db, want['enc_db'])
    Q, ldi = P * T * R, xh_width(H)
    dW0 = f32(np.random.default_rng(5).standard_normal((2 * H, 4 * H)))
    dW = dW0.copy()
    scratch = np.zeros(lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, H, ldi), np.float32)
    check(lib.ic3_lstm_weight_grad_wide(p(win.inp), ldi, p(win.hsl), p(dgates), None, Q, H, p(dW), 1, 1, p(scratch), None))
    errs['dW'] = ref.rel_err(dW, dW0.astype(np.float64) + want['dW'])
    env.close()
    ref.check('host/' + name, errs)


def test_what_the_two_entries_refuse():
    """The recording pass: no split planes -> -ENOSYS, a null output -> -EINVAL, another struct_size -> -EINVAL before
    anything else is read; the passes window: another struct_size of its descriptor, passes < 2."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    H, N, E = 64, 3, 2
    P64 = make_params(12, H, HEADS, seed=1, comm_passes=2)
    plain = HostPolicy(None, P64, H, HEADS, use_table=False, inner=True)
    split = HostPolicy(None, P64, H, HEADS, use_table=False, inner=True, gate_split=True)
    z = lambda *s: np.zeros(s, np.float32)
    enc, h, c, g, x = z(E * N, H), z(E * N, H), z(E * N, H), z(E * N, 4 * H), z(E * N, 2 * H)
    if not plain.struct.gate_split:                              # (IC3_HOST_FORCE_SPLIT=1 gives every policy the planes)
        assert forward_record(plain, enc, None, E, N, h, c, h, c, None, None, g, x) == -38
        assert b"gate_split" in lib.ic3_last_error()
    assert forward_record(split, enc, None, E, N, h, c, h, None, None, None, g, x) == -22
    assert forward_record(split, enc, None, E, N, h, c, h, c, None, None, g, x) == 0
    split.size_off = 8
    assert forward_record(split, enc, None, E, N, h, c, h, c, None, None, g, x) == -22 and b"struct_size" in lib.ic3_last_error()
    g[:] = np.nan                                                # a plain ic3_policy carrying the tag: refused by its size, nothing written
    tagged = binding.Policy()
    C.memmove(C.addressof(tagged), C.addressof(split.struct), C.sizeof(tagged))
    tagged.inner_pass = binding.PolicyRecord.RECORD_PASS
    assert lib.ic3_policy_forward(C.byref(tagged), p(enc), E, N, p(h), p(c), None, None, None, None) == -22 and np.isnan(g).all()
    env = HostEnv.pp(3, 6, 1, 'mixed', E, seed=3)
    b = binding.BpttPasses(1, E, N, H, OT, 2)
    b.struct_size -= 8
    assert passes_backward(lib, env, b) == -22 and b"ic3_bptt_passes has" in lib.ic3_last_error()
    b = binding.BpttPasses(1, E, N, H, OT, 1)
    assert passes_backward(lib, env, b) == -22 and b"passes >= 2" in lib.ic3_last_error()
    env.close()

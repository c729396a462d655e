"""CPU: ic3_bptt_backward on an ic3_bptt_passes descriptor with the collection-mode row factors (row_keep / keep_before) on the host
build of the product's own sources (tests/host/libic3rollout_host.so), against the float64 collection-mode window backward of
tests/bptt_passes_stream_ref.py.  The cases, what the caller does around the call and the assertions are those of
tests/bptt_passes_stream_cases.py (shared with the GPU test); this file is the host backend — ctypes on numpy arrays — and the
refusals."""
import ctypes as C

import numpy as np
import pytest

import bptt_passes_stream_cases as cases
from host_abi_util import HostEnv, check, host_lib, p

f32 = cases.f32
arr = lambda xs: C.cast((C.c_void_p * len(xs))(*[None if a is None else a.ctypes.data for a in xs]), C.POINTER(C.c_void_p))


def make_env(spec):
    kind, N, dim, E = spec
    if kind == 'pp':
        return HostEnv.pp(N, dim, 1, 'mixed', E, seed=3)
    return HostEnv.tj(N, dim, 1, 'easy', E, seed=3, add_rate_min=0.6, add_rate_max=0.6)


def snapshots(env, T):
    from test_host_abi_cpu import _play
    snaps, obs = [], []
    for t in range(T):
        _play(env, 2 + t, 70 + t)
        snaps.append(env.snapshot())
        obs.append(env.observe().reshape(env.E * env.N, env.obs_dim).astype(np.float64))
    return np.ascontiguousarray(np.stack(snaps)), obs


class Call(object):
    """The descriptor of one call on slots [t0, t1) of a case's arrays; the arrays it points into are kept alive here."""

    def __init__(self, lib, env, case, bufs, t0, t1, first, factors=True, gap=0):
        from ic3net_amd import _lib as binding
        P, R, H = case.P, case.R, case.H
        self.b = b = binding.BpttPasses(t1 - t0, case.E, case.N, H, cases.OT, P, int(case.avg), int(case.comm_zero), gap, int(first), t0)
        self.keep = dict(gates=arr([bufs['dgates'][i, t0:t1] for i in range(P)]), hs=arr([case.hs_in[i, t0:t1] for i in range(P)]),
                         cs=arr([case.cs_in[i, t0:t1] for i in range(P)]), dxh=arr([bufs['dxh'][i, t0:t1] for i in range(P)]),
                         dbias_partials=arr([bufs['bias'][i] for i in range(P)]))
        if not case.comm_zero:
            self.keep.update(dcw_partials=arr([bufs['dcw'][i] for i in range(P)]), c_weight=arr(case.w['c_weights']))
        if case.alive is not None:
            self.keep['alive'] = arr(case.alive[t0:t1])
        if case.gate is not None:
            self.keep['gate'] = arr(case.gate[t0:t1])
        for k, v in self.keep.items():
            setattr(b, k, v)
        b.dhead, b.snaps, b.snap_words = case.w['dhead'][t0:t1].ctypes.data, bufs['snaps'][t0:t1].ctypes.data, bufs['snaps'].shape[1]
        b.lstm_wp3_bwd, b.w_heads = bufs['wb3'].ctypes.data, case.w['w_heads'].ctypes.data
        b.dh, b.dc = bufs['dh'].ctypes.data, bufs['dc'].ctypes.data
        b.dxh_step, b.enc_work = R * 2 * H, bufs['work'].ctypes.data
        if factors:
            b.row_keep = case.keep_rows[t0:t1].ctypes.data
            b.keep_before = case.keep_rows[t0 - 1].ctypes.data if t0 > 0 else None
        self.lib, self.env = lib, env

    def __call__(self):
        return self.lib.ic3_bptt_backward(self.env._h, C.byref(self.b), None)


def buffers(lib, env, case, snaps):
    P, T, R, H = case.P, case.T, case.R, case.H
    slots = lib.ic3_comm_backward_partials(case.E, case.N)
    bufs = dict(dgates=case.w['gates'].copy(), dxh=np.full((P, T, R, 2 * H), np.nan, np.float32), dh=case.dh_in.copy(),
                dc=case.w['dc'].copy(), bias=case.bias0.copy(), snaps=snaps,
                dcw0=None if case.comm_zero else f32(np.random.default_rng(98).standard_normal((P, slots, H, H))),
                wb3=np.zeros(3 * 4 * H * 2 * H, np.uint16))
    bufs['dcw'] = None if case.comm_zero else bufs['dcw0'].copy()
    check(lib.ic3_policy_pack_split_bwd(p(case.w['w_ih']), p(case.w['w_hh']), p(bufs['wb3']), H, None))
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H))
    assert n > 0 and lib.ic3_bptt_backward_supported(env._h, H) == 1
    bufs['work'] = np.full((n,), np.nan, np.float32)
    return bufs


def run(case, most):
    lib = host_lib()
    env = make_env(case.cfg['env'])
    assert (env.E, env.N) == (case.E, case.N)
    snaps, obs = snapshots(env, case.T)
    bufs = buffers(lib, env, case, snaps)
    first = True
    for t0, t1 in cases.chunks(case.T, most or case.T):
        check(Call(lib, env, case, bufs, t0, t1, first)())
        first = False
    P, T, R, H = case.P, case.T, case.R, case.H
    dwt, db = np.full((env.obs_dim, H), np.nan, np.float32), np.full((H,), np.nan, np.float32)
    check(lib.ic3_env_encode_backward_window_finish(env._h, H, p(dwt), p(db), p(bufs['work']), None))
    Q = P * T * R
    dW = case.dW0.copy()
    scratch = np.zeros(lib.ic3_lstm_weight_grad_wide_scratch_floats(Q, H, H), np.float32)
    check(lib.ic3_lstm_weight_grad_wide(p(case.w['inp']), H, p(case.hs_in), p(bufs['dgates']), None, Q, H, p(dW), 1, 1, p(scratch), None))
    env.close()
    return dict(bufs, enc_dwt=dwt, enc_db=db, dW=dW), obs


@pytest.mark.parametrize("name", list(cases.CASES))
def test_passes_backward_with_row_factors_against_float64(name):
    """Every buffer the call writes or adds to — dgates of every (slot, pass), the dxh rings, dh / dc leaving the window, every row
    of each pass's bias partials (and C_i.bias's gradient read off them), each pass's dcw sum, the encoder's dWt / db through the
    window finish, dW of ic3_lstm_weight_grad_wide over the P x T x R rows (pass 0's h rows: the zeroed copies) — for the window in
    one call and in chunks of 2 slots, each against the float64 reference of the WHOLE window at its bar."""
    cases.run_and_check('host', name, run)


def _small(gap=0, factors=True):
    lib = host_lib()
    case = cases.Case('h64-tj-n5-E13-T4-P2-comm-zero-independent')
    env = make_env(case.cfg['env'])
    snaps, _ = snapshots(env, case.T)
    bufs = buffers(lib, env, case, snaps)
    return lib, env, case, bufs, Call(lib, env, case, bufs, 0, case.T, True, factors=factors, gap=gap)


def test_detach_gap_with_row_factors_is_refused_before_the_first_launch():
    """detach_gap > 0 with row_keep, and with keep_before alone: -EINVAL, and gates, dh, dc, the partials keep their bits, the rings
    stay unwritten."""
    lib, env, case, bufs, call = _small(gap=2)
    call.b.keep_before = case.keep_rows[0].ctypes.data
    for drop in (None, 'row_keep'):
        if drop:
            setattr(call.b, drop, None)
        assert call() == -22 and b"detach_gap > 0 with row_keep" in lib.ic3_last_error()
        np.testing.assert_array_equal(bufs['dgates'], case.w['gates'])
        np.testing.assert_array_equal(bufs['dh'], case.dh_in)
        np.testing.assert_array_equal(bufs['dc'], case.w['dc'])
        np.testing.assert_array_equal(bufs['bias'], case.bias0)
        assert np.isnan(bufs['dxh']).all()
    call.b.keep_before = None                                    # no factor left: the lock-step call, detach points and all
    assert call() == 0
    env.close()


def test_the_descriptor_without_the_factor_fields_is_refused():
    """The struct as it was before the two pointers were appended (16 bytes shorter), and 8 bytes shorter: -EINVAL by its size"""
    lib, env, case, bufs, call = _small()
    full = call.b.struct_size
    for less in (16, 8):
        call.b.struct_size = full - less
        assert call() == -22 and b"ic3_bptt_passes has" in lib.ic3_last_error()
        np.testing.assert_array_equal(bufs['dgates'], case.w['gates'])
    env.close()


def test_null_factors_are_the_call_without_them():
    """row_keep = keep_before = NULL against the same call with every factor 1.0 (a window nothing cuts): the same bits in every
    buffer — and different bits from the case's real factors (the comparison is not vacuous)."""
    outs = []
    for mode in ('null', 'ones', 'real'):
        lib, env, case, bufs, call = _small(factors=mode != 'null')
        ones = np.ones_like(case.keep_rows)
        if mode == 'ones':
            call.b.row_keep, call.b.keep_before = ones.ctypes.data, ones[0].ctypes.data
        assert call() == 0
        outs.append(bufs)
        env.close()
    for k in ('dgates', 'dxh', 'dh', 'dc', 'bias'):
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
    assert not np.array_equal(outs[0]['dgates'], outs[2]['dgates']) and not np.array_equal(outs[0]['dh'], outs[2]['dh'])

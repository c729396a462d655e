"""CPU: ic3_bptt_backward on an ic3_bptt_passes descriptor handed slices of a window-long per-pass record — gates[i][t0:t1],
hs[i][t0:t1], cs[i][t0:t1] of (P, T, R, .) arrays, consecutive passes a whole window apart — against the same chunks copied into
contiguous rings (P, Tc, R, .), on the host build (tests/host).  Both must give the same dgates, dxh, dh, dc and partials BIT FOR
BIT.  Shape h64-n3-E5-T3-P2-gap2 (tests/test_host_bptt_passes_cpu.py), walked in chunks of 2 of 3 steps, last chunk first.  (This
guards the caller that reads the window launch's record, args.window_record_passes; the call itself is unchanged.)"""
import ctypes as C

import numpy as np

import bptt_passes_ref as ref
from host_abi_util import HostEnv, check, host_lib, p

OT = 8


def _run(env, w, snaps, layout, chunk):
    from ic3net_amd import _lib as binding
    lib = host_lib()
    T, E, N, H, P = w['T'], w['E'], w['N'], w['H'], w['P']
    R = E * N
    gates, hs, cs = w['gates'].copy(), w['hs'].copy(), w['cs'].copy()      # (P, T, R, .): the record
    dh, dc = w['dh'].copy(), w['dc'].copy()
    nan = lambda *s: np.full(s, np.nan, np.float32)
    ring = dict(gates=nan(P, chunk, R, 4 * H), hs=nan(P, chunk, R, H), cs=nan(P, chunk, R, H))
    dxh = nan(P, chunk, R, 2 * H)
    rng = np.random.default_rng(99)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    bias = f32(rng.standard_normal((P, (R + 63) // 64, 4 * H)))
    dcw = f32(rng.standard_normal((P, lib.ic3_comm_backward_partials(E, N), H, H)))
    wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
    check(lib.ic3_policy_pack_split_bwd(p(w['w_ih']), p(w['w_hh']), p(wb3), H, None))
    work = nan(int(lib.ic3_env_encode_backward_window_work(env._h, H)))
    arr = lambda xs: C.cast((C.c_void_p * len(xs))(*[None if a is None else a.ctypes.data for a in xs]), C.POINTER(C.c_void_p))
    out = dict(dgates=nan(P, T, R, 4 * H), dxh=nan(P, T, R, 2 * H))
    first = True
    for t1 in range(T, 0, -chunk):
        t0 = max(t1 - chunk, 0)
        Tn = t1 - t0
        if layout == 'ring':
            for k, src in (('gates', gates), ('hs', hs), ('cs', cs)):
                ring[k][:, :Tn] = src[:, t0:t1]
            g_p, h_p, c_p = ([ring[k][i, :Tn] for i in range(P)] for k in ('gates', 'hs', 'cs'))
        else:
            g_p, h_p, c_p = ([src[i, t0:t1] for i in range(P)] for src in (gates, hs, cs))
            assert g_p[1].ctypes.data - g_p[0].ctypes.data == T * R * 4 * H * 4 and all(a.flags['C_CONTIGUOUS'] for a in g_p + h_p + c_p)
        b = binding.BpttPasses(Tn, E, N, H, OT, P, 1, 0, 2, int(first), t0)
        keep = dict(gates=arr(g_p), hs=arr(h_p), cs=arr(c_p), dxh=arr([dxh[i] for i in range(P)]),
                    dbias_partials=arr([bias[i] for i in range(P)]), dcw_partials=arr([dcw[i] for i in range(P)]),
                    c_weight=arr(w['c_weights']), gate=arr(w['gate'][t0:t1]), alive=arr(w['alive'][t0:t1]))
        for k, v in keep.items():
            setattr(b, k, v)
        dhead, sn = np.ascontiguousarray(w['dhead'][t0:t1]), np.ascontiguousarray(snaps[t0:t1])
        b.dhead, b.snaps, b.snap_words = dhead.ctypes.data, sn.ctypes.data, sn.shape[1]
        b.lstm_wp3_bwd, b.w_heads, b.dh, b.dc = wb3.ctypes.data, w['w_heads'].ctypes.data, dh.ctypes.data, dc.ctypes.data
        b.dxh_step, b.enc_work = R * 2 * H, work.ctypes.data
        check(lib.ic3_bptt_backward(env._h, C.byref(b), None))
        first = False
        for i in range(P):
            out['dgates'][i, t0:t1] = g_p[i]
            out['dxh'][i, t0:t1] = dxh[i, :Tn]
    out.update(dh=dh, dc=dc, bias=bias, dcw=dcw)
    return out


def test_record_slices_give_the_bits_of_the_contiguous_rings():
    from test_host_abi_cpu import _play
    name = 'h64-n3-E5-T3-P2-gap2'
    env = HostEnv.pp(3, 6, 1, 'mixed', 5, seed=3)
    T, H, P, E, N = 3, 64, 2, env.E, env.N
    w = ref.make_window(sum(map(ord, name)), T, E, N, H, OT, P, alive='first_null')
    snaps = []
    for t in range(T):
        _play(env, 2 + t, 70 + t)
        snaps.append(env.snapshot())
    snaps = np.ascontiguousarray(np.stack(snaps))
    a, b = _run(env, w, snaps, 'ring', 2), _run(env, w, snaps, 'slices', 2)
    env.close()
    for k in ('dgates', 'dxh', 'dh', 'dc', 'bias', 'dcw'):
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)
        assert np.isfinite(a[k]).all(), k
    assert not np.array_equal(a['dgates'], w['gates']), "the backward wrote no dgates"

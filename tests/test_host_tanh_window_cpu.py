"""CPU: ic3_rnn_backward and ic3_mlp_backward — the tanh-recurrence and the IC baseline's window backwards as ONE host call each —
on the host build of the product's own sources (tests/host/libic3rollout_host.so) against the float64 window backwards of
tests/tanh_window_ref.py: which slot of the record a step reads h_t from, which step's row_keep scales what crosses, which steps
are detached, dh in place over the steps, the partials and a2_grad added to across steps and windows, row_live in the weight
gradient, both encoder forms and enc_first over a second window; the IC call's rings, its skip term and its table encoder."""
import ctypes as C

import numpy as np
import pytest

import tanh_window_ref as ref
from host_abi_util import HostEnv, check, host_lib, p


def _env(kind, E):
    if kind == 'pp':
        return HostEnv.pp(3, 6, 1, 'mixed', E, seed=3)
    return HostEnv.tj(5, 6, 1, 'easy', E, seed=3, add_rate_min=0.6, add_rate_max=0.6)


def _record_states(env, T):
    """T snapshots of random play (restarted with another seed and length each) and their dense observations in float64"""
    from test_host_abi_cpu import _play
    snaps, obs = [], []
    for t in range(T):
        _play(env, 2 + t, 70 + t)
        snaps.append(env.snapshot())
        obs.append(env.observe().reshape(env.E * env.N, env.obs_dim).astype(np.float64))
    return np.ascontiguousarray(np.stack(snaps)), obs


def _enc_work(lib, env, H, enc_window):
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H) if enc_window else lib.ic3_env_encode_backward_work(env._h, H))
    assert n > 0
    return np.full((n,), np.nan, np.float32)


def _enc_finish(lib, env, H, work, enc_window, ordered=False):
    dwt = np.full((env.obs_dim, H), np.nan, np.float32)
    db = np.full((H,), np.nan, np.float32)
    if ordered:
        fold = np.full((lib.ic3_env_encode_backward_window_finish_scratch(env._h, H),), np.nan, np.float32)
        check(lib.ic3_env_encode_backward_window_finish_ordered(env._h, H, p(dwt), p(db), p(work), p(fold), None))
    else:
        fin = lib.ic3_env_encode_backward_window_finish if enc_window else lib.ic3_env_encode_backward_finish
        check(fin(env._h, H, p(dwt), p(db), p(work), None))
    return dwt, db


RNN_CASES = {
    # A: lock-step at hid 64, R = 150 = two tiles + 22 rows; T = 5 with detach_gap = 2 detaches steps 1 and 3 inside the window; the
    #    last step's h_t in a buffer of its own; the encoder's window form
    'rnn-A-h64-T5-gap2-h-last': dict(kind='pp', E=50, H=64, T=5, gap=2, h_last='separate'),
    # A4: T = 4 with detach_gap = 2 detaches the window's last step (the arriving dh counts for nothing)
    'rnn-A4-h64-T4-gap2': dict(kind='pp', E=50, H=64, T=4, gap=2),
    # B: collection cuts on Traffic-Junction, the per-step encoder form, T + 1 slots, the widest heads
    'rnn-B-h64-collect-per-step-OT16': dict(kind='tj', E=30, H=64, T=4, collect=True, enc_window=False, OT=16),
    # C: two windows of 3 steps back to back on one set of accumulators (the later window first: enc_first = 1, then 0), the dh the
    #    first call left times the row_keep of the border (the caller's part) into the second; the reference runs the 6 steps once
    'rnn-C-h64-collect-two-windows': dict(kind='pp', E=50, H=64, T=6, collect=True, windows=((3, 3), (0, 3))),
    'rnn-C2-h64-collect-two-windows-per-step': dict(kind='tj', E=30, H=64, T=4, collect=True, windows=((2, 2), (0, 2)), enc_window=False),
    # D: hid 128, R = 90 = one tile + 26 rows
    'rnn-D-h128-T3-gap2': dict(kind='pp', E=30, H=128, T=3, gap=2),
    # E: a one-step window that is all detach, the single-column heads, no weight gradient
    'rnn-E-h64-T1-gap1-OT1': dict(kind='pp', E=9, H=64, T=1, gap=1, OT=1, a2=False),
}


@pytest.mark.parametrize("name", list(RNN_CASES))
def test_rnn_window_backward_against_float64(name):
    """Every slot of the dz ring, dh leaving the window, the partials' column sum and EVERY partial row (one per tile at these
    sizes) on top of their known pre-fill, a2_grad on top of its pre-fill, and the encoder's dWt / db through the finish that goes
    with the form — each against the float64 window backward at its bar (tanh_window_ref.check)."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    cfg = RNN_CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, H, OT, gap = cfg['T'], cfg['H'], cfg.get('OT', 6), cfg.get('gap', 0)
    E, N = env.E, env.N
    R = E * N
    enc_window = cfg.get('enc_window', True)
    w = ref.make_rnn_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False), h_last=cfg.get('h_last', 'slot'))
    snaps, obs = _record_states(env, T)
    want = ref.rnn_reference_of(w, obs=obs, detach_gap=gap)
    rng = np.random.default_rng(99)
    nparts = lib.ic3_rnn_backward_partials(R, H)
    assert nparts == (R + 63) // 64
    parts0 = rng.standard_normal((nparts, H)).astype(np.float32)
    a2g0 = rng.standard_normal((H, H)).astype(np.float32)
    parts, a2g, dh = parts0.copy(), a2g0.copy(), w['dh'].copy()
    dz = np.full((T, R, H), np.nan, np.float32)
    work = _enc_work(lib, env, H, enc_window)
    windows = cfg.get('windows', ((0, T),))
    for k, (t0, n) in enumerate(windows):
        b = binding.RnnBptt()
        b.struct_size = C.sizeof(b)
        b.T, b.E, b.N, b.H, b.OT = n, E, N, H, OT
        b.detach_gap, b.enc_first, b.enc_window = gap, int(k == 0), int(enc_window)
        hs, dhead, sn, ring = w['hs'][t0:], w['dhead'][t0:t0 + n], snaps[t0:t0 + n], dz[t0:t0 + n]
        b.hs, b.dhead, b.snaps, b.snap_words = hs.ctypes.data, dhead.ctypes.data, sn.ctypes.data, snaps.shape[1]
        b.h_last = w['h_last'].ctypes.data if (w['h_last'] is not None and t0 + n == T) else None
        b.a2, b.w_heads = w['a2'].ctypes.data, w['w_heads'].ctypes.data
        if w['row_live'] is not None:
            live, keep = w['row_live'][t0:t0 + n], w['row_keep'][t0:t0 + n]
            b.row_live, b.row_keep = live.ctypes.data, keep.ctypes.data
            if k:                                                # (the caller's part: what crosses the border between two windows)
                dh *= w['row_keep'][t0 + n - 1][:, None]
        b.dh, b.dz, b.dbias_partials, b.enc_work = dh.ctypes.data, ring.ctypes.data, parts.ctypes.data, work.ctypes.data
        if cfg.get('a2', True):
            scratch = np.full(lib.ic3_rnn_weight_grad_scratch_floats(n * R, H), np.nan, np.float32)
            b.a2_grad, b.wgrad_scratch = a2g.ctypes.data, scratch.ctypes.data
        check(lib.ic3_rnn_backward(env._h, C.byref(b), None))
    errs = ref.rnn_errors(want, dz, dh, parts, parts0, a2g if cfg.get('a2', True) else None, a2g0)
    assert 'dbias_tiles' in errs
    if not cfg.get('a2', True):
        np.testing.assert_array_equal(a2g, a2g0)
    dwt, db = _enc_finish(lib, env, H, work, enc_window)
    errs['enc_dwt'], errs['enc_db'] = ref.rel_err(dwt, want['enc_dwt']), ref.rel_err(db, want['enc_db'])
    env.close()
    ref.check('host/' + name, errs)


MLP_CASES = {
    # A: hid 128, Q = 2 x 90 = 180 rows: three tiles, the second spans both steps' rows, the last is ragged
    'mlp-A-h128-T2': dict(kind='pp', E=30, H=128, T=2),
    # B: hid 64, Q = 3 x 150 = 450 rows = 7 tiles + 2 rows, the table form of the encoder, the widest heads; a second window on the
    #    same accumulators (enc_first = 0)
    'mlp-B-h64-T3-table-OT16-two-windows': dict(kind='tj', E=30, H=64, T=3, table=True, OT=16, windows=2),
    # C: the per-step encoder form
    'mlp-C-h64-T2-per-step': dict(kind='pp', E=30, H=64, T=2, enc_window=False),
}


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_window_backward_against_float64(name):
    """The x1 / dz / de rings, the partials from a NaN pre-fill (column sum and every row: one per tile here), a2_grad on top of its
    pre-fill and the encoder's dWt / db through the finishes that go with the form (window form: ordered and plain) — against the
    float64 window backward at its bar; with `windows` = 2 the same window once more with enc_first = 0: the rings and partials
    written again, a2_grad and the encoder's sums twice the window's."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    cfg = MLP_CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, H, OT = cfg['T'], cfg['H'], cfg.get('OT', 6)
    E, N = env.E, env.N
    R = E * N
    Q = T * R
    enc_window, windows = cfg.get('enc_window', True), cfg.get('windows', 1)
    w = ref.make_mlp_window(sum(map(ord, name)), T, E, N, H, OT, env.obs_dim)
    snaps, obs = _record_states(env, T)
    want = ref.mlp_reference_of(w, obs)
    table = env.encode_table(w['enc_wt']) if cfg.get('table') else None
    nparts = lib.ic3_mlp_backward_partials(Q, H)
    assert nparts == (Q + 63) // 64 and nparts >= 3
    a2g0 = np.random.default_rng(99).standard_normal((H, H)).astype(np.float32)
    a2g = a2g0.copy()
    work = _enc_work(lib, env, H, enc_window)
    scratch = np.full(lib.ic3_rnn_weight_grad_scratch_floats(Q, H), np.nan, np.float32)
    for k in range(windows):
        x1, dz, de = (np.full((T, R, H), np.nan, np.float32) for _ in range(3))
        parts = np.full((nparts, H), np.nan, np.float32)
        b = binding.MlpBptt()
        b.struct_size = C.sizeof(b)
        b.T, b.E, b.N, b.H, b.OT = T, E, N, H, OT
        b.enc_first, b.enc_window = int(k == 0), int(enc_window)
        b.h, b.dhead, b.snaps, b.snap_words = w['h'].ctypes.data, w['dhead'].ctypes.data, snaps.ctypes.data, snaps.shape[1]
        b.enc_wt, b.enc_bias = w['enc_wt'].ctypes.data, w['enc_bias'].ctypes.data
        b.loc_table = table.ctypes.data if table is not None else None
        b.a2, b.w_heads = w['a2'].ctypes.data, w['w_heads'].ctypes.data
        b.x1, b.dz, b.de, b.dbias_partials = x1.ctypes.data, dz.ctypes.data, de.ctypes.data, parts.ctypes.data
        b.enc_work, b.a2_grad, b.wgrad_scratch = work.ctypes.data, a2g.ctypes.data, scratch.ctypes.data
        check(lib.ic3_mlp_backward(env._h, C.byref(b), None))
    errs = ref.mlp_errors(want, x1, dz, de, parts, a2g, a2g0, windows=windows)
    assert 'dbias_tiles' in errs
    for ordered in ((True, False) if enc_window else (False,)):
        dwt, db = _enc_finish(lib, env, H, work, enc_window, ordered=ordered)
        tag = '_ordered' if ordered else ''
        errs['enc_dwt' + tag] = ref.rel_err(dwt, windows * want['enc_dwt'])
        errs['enc_db' + tag] = ref.rel_err(db, windows * want['enc_db'])
    env.close()
    ref.check('host/' + name, errs)

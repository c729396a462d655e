"""CPU: the tanh-recurrence and the IC baseline's window backwards at hid 256 — ic3_rnn_backward_wide, ic3_mlp_backward_wide and
ic3_rnn_weight_grad_wide (include/ic3_rollout.h) — on the host build of the product's own sources (tests/host/libic3rollout_host.so)
against the float64 window backwards of tests/tanh_window_ref.py (they do not depend on H), each quantity at its bar from
tests/tanh_window_h256_bars.py; and the contract of the _wide twins beside the 64 / 128 entries."""
import ctypes as C

import numpy as np
import pytest

import tanh_window_ref as ref
from host_abi_util import HostEnv, check, host_lib, p
from tanh_window_h256_bars import check as check_bars
from test_host_tanh_window_cpu import _enc_finish, _enc_work, _env, _record_states

H = 256

RNN_CASES = {
    # A: lock-step, R = 90 = one tile + 26 rows; T = 3 with detach_gap = 2 detaches step 1 inside the window; the encoder's window form
    'rnn-A-h256-T3-gap2': dict(kind='pp', E=30, T=3, gap=2),
    # B: collection cuts over two windows of 2 steps on one set of accumulators (the later window first: enc_first = 1, then 0), the
    #    dh the first call left times the row_keep of the border into the second; the reference runs the 4 steps once
    'rnn-B-h256-collect-two-windows': dict(kind='pp', E=30, T=4, collect=True, windows=((2, 2), (0, 2))),
    # C: the widest heads, the per-step encoder form, the last step's h_t in a buffer of its own
    'rnn-C-h256-T3-per-step-OT16-h-last': dict(kind='tj', E=30, T=3, enc_window=False, OT=16, h_last='separate'),
}


@pytest.mark.parametrize("name", list(RNN_CASES))
def test_rnn_window_backward_h256_against_float64(name):
    """Every slot of the dz ring, dh leaving the window, the partials' column sum and every partial row (one per tile at these
    sizes: a row-owning workgroup's sums over all 256 columns) on top of their pre-fill, a2_grad on top of its pre-fill, and the
    encoder's dWt / db through the finish that goes with the form."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    cfg = RNN_CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, OT, gap = cfg['T'], cfg.get('OT', 6), cfg.get('gap', 0)
    E, N = env.E, env.N
    R = E * N
    enc_window = cfg.get('enc_window', True)
    w = ref.make_rnn_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False), h_last=cfg.get('h_last', 'slot'))
    snaps, obs = _record_states(env, T)
    want = ref.rnn_reference_of(w, obs=obs, detach_gap=gap)
    rng = np.random.default_rng(99)
    nparts = lib.ic3_rnn_backward_wide_partials(R, H)
    assert nparts == (R + 63) // 64 and R % 64
    parts0 = rng.standard_normal((nparts, H)).astype(np.float32)
    a2g0 = rng.standard_normal((H, H)).astype(np.float32)
    parts, a2g, dh = parts0.copy(), a2g0.copy(), w['dh'].copy()
    dz = np.full((T, R, H), np.nan, np.float32)
    work = _enc_work(lib, env, H, enc_window)
    for k, (t0, n) in enumerate(cfg.get('windows', ((0, T),))):
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
        scratch = np.full(lib.ic3_rnn_weight_grad_wide_scratch_floats(n * R, H), np.nan, np.float32)
        b.a2_grad, b.wgrad_scratch = a2g.ctypes.data, scratch.ctypes.data
        check(lib.ic3_rnn_backward_wide(env._h, C.byref(b), None))
    errs = ref.rnn_errors(want, dz, dh, parts, parts0, a2g, a2g0)
    assert 'dbias_tiles' in errs
    dwt, db = _enc_finish(lib, env, H, work, enc_window)
    errs['enc_dwt'], errs['enc_db'] = ref.rel_err(dwt, want['enc_dwt']), ref.rel_err(db, want['enc_db'])
    env.close()
    check_bars('host/' + name, errs)


MLP_CASES = {
    # A: Q = 2 x 90 = 180 rows: three tiles, the second spans both steps' rows, the last is ragged
    'mlp-A-h256-T2': dict(kind='pp', E=30, T=2),
    # B: the table form of the encoder; the same window once more on the same a2_grad and encoder sums (enc_first = 0)
    'mlp-B-h256-T2-table-two-windows': dict(kind='tj', E=20, T=2, table=True, windows=2),
}


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_window_backward_h256_against_float64(name):
    """The x1 / dz / de rings, the partials from a NaN pre-fill (column sum and every row: one per tile here), a2_grad on top of its
    pre-fill and the encoder's dWt / db through both finishes of the window form; with `windows` = 2 the same window once more with
    enc_first = 0: the rings and partials written again, a2_grad and the encoder's sums twice the window's."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    cfg = MLP_CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, OT = cfg['T'], cfg.get('OT', 6)
    E, N = env.E, env.N
    R = E * N
    Q = T * R
    windows = cfg.get('windows', 1)
    w = ref.make_mlp_window(sum(map(ord, name)), T, E, N, H, OT, env.obs_dim)
    snaps, obs = _record_states(env, T)
    want = ref.mlp_reference_of(w, obs)
    table = env.encode_table(w['enc_wt']) if cfg.get('table') else None
    nparts = lib.ic3_mlp_backward_wide_partials(Q, H)
    assert nparts == (Q + 63) // 64 and nparts >= 2 and Q % 64
    a2g0 = np.random.default_rng(99).standard_normal((H, H)).astype(np.float32)
    a2g = a2g0.copy()
    work = _enc_work(lib, env, H, True)
    scratch = np.full(lib.ic3_rnn_weight_grad_wide_scratch_floats(Q, H), np.nan, np.float32)
    for k in range(windows):
        x1, dz, de = (np.full((T, R, H), np.nan, np.float32) for _ in range(3))
        parts = np.full((nparts, H), np.nan, np.float32)
        b = binding.MlpBptt()
        b.struct_size = C.sizeof(b)
        b.T, b.E, b.N, b.H, b.OT = T, E, N, H, OT
        b.enc_first, b.enc_window = int(k == 0), 1
        b.h, b.dhead, b.snaps, b.snap_words = w['h'].ctypes.data, w['dhead'].ctypes.data, snaps.ctypes.data, snaps.shape[1]
        b.enc_wt, b.enc_bias = w['enc_wt'].ctypes.data, w['enc_bias'].ctypes.data
        b.loc_table = table.ctypes.data if table is not None else None
        b.a2, b.w_heads = w['a2'].ctypes.data, w['w_heads'].ctypes.data
        b.x1, b.dz, b.de, b.dbias_partials = x1.ctypes.data, dz.ctypes.data, de.ctypes.data, parts.ctypes.data
        b.enc_work, b.a2_grad, b.wgrad_scratch = work.ctypes.data, a2g.ctypes.data, scratch.ctypes.data
        check(lib.ic3_mlp_backward_wide(env._h, C.byref(b), None))
    errs = ref.mlp_errors(want, x1, dz, de, parts, a2g, a2g0, windows=windows)
    assert 'dbias_tiles' in errs
    for ordered in (True, False):
        dwt, db = _enc_finish(lib, env, H, work, True, ordered=ordered)
        tag = '_ordered' if ordered else ''
        errs['enc_dwt' + tag] = ref.rel_err(dwt, windows * want['enc_dwt'])
        errs['enc_db' + tag] = ref.rel_err(db, windows * want['enc_db'])
    env.close()
    check_bars('host/' + name, errs)


def test_rnn_weight_grad_wide_h256_ragged_rows_row_live_accumulate():
    """ic3_rnn_weight_grad_wide alone at hid 256: Q = 203 rows (no multiple of 16, nor of the K slices), h rows times row_live;
    accumulate = 0 over a NaN dA2, then accumulate = 1 on top: twice the product.  The scratch is slices x 256 x 256 floats."""
    lib = host_lib()
    Q = 203
    rng = np.random.default_rng(5)
    dz = rng.standard_normal((Q, H)).astype(np.float32)
    h = np.tanh(rng.standard_normal((Q, H))).astype(np.float32)
    live = (rng.random(Q) < 0.8).astype(np.float32)
    want = dz.astype(np.float64).T @ (h.astype(np.float64) * live[:, None])
    n = lib.ic3_rnn_weight_grad_wide_scratch_floats(Q, H)
    assert n > 0 and n % (H * H) == 0
    scratch = np.full(n, np.nan, np.float32)
    dA2 = np.full((H, H), np.nan, np.float32)
    ks = check(lib.ic3_rnn_weight_grad_wide(p(dz), p(h), p(live), Q, H, p(dA2), 0, p(scratch), None))
    assert ks == n // (H * H) and Q % ks and Q % 16
    errs = dict(a2_grad=ref.rel_err(dA2, want))
    first = dA2.copy()
    assert check(lib.ic3_rnn_weight_grad_wide(p(dz), p(h), p(live), Q, H, p(dA2), 1, p(scratch), None)) == ks
    np.testing.assert_array_equal(dA2, first + first)
    errs['a2_grad_accumulated'] = ref.rel_err(dA2, 2 * want)
    check_bars('host/wgrad-h256-Q203-row-live', errs)


def test_wide_twins_contract():
    """The _wide queries answer 1 / > 0 at 64, 128 and 256 and 0 at 32 and 96; at 64 / 128 they equal the earlier queries, which
    still answer 0 at 256; the _wide calls refuse other sizes with -ENOSYS and a descriptor of another size with -EINVAL first."""
    from ic3net_amd import _lib as binding
    lib = host_lib()
    env = _env('pp', 9)
    R = env.E * env.N
    for Hq in (64, 128, 256):
        assert lib.ic3_rnn_backward_wide_supported(env._h, Hq) == 1 and lib.ic3_mlp_backward_wide_supported(env._h, Hq) == 1
        assert lib.ic3_rnn_backward_wide_partials(R, Hq) > 0 and lib.ic3_mlp_backward_wide_partials(5 * R, Hq) > 0
        assert lib.ic3_rnn_weight_grad_wide_scratch_floats(5 * R, Hq) > 0
    for Hq in (64, 128):
        assert lib.ic3_rnn_backward_wide_supported(env._h, Hq) == lib.ic3_rnn_backward_supported(env._h, Hq)
        assert lib.ic3_mlp_backward_wide_supported(env._h, Hq) == lib.ic3_mlp_backward_supported(env._h, Hq)
        for rows in (R, 5 * R, 100000):
            assert lib.ic3_rnn_backward_wide_partials(rows, Hq) == lib.ic3_rnn_backward_partials(rows, Hq)
            assert lib.ic3_mlp_backward_wide_partials(rows, Hq) == lib.ic3_mlp_backward_partials(rows, Hq)
            assert lib.ic3_rnn_weight_grad_wide_scratch_floats(rows, Hq) == lib.ic3_rnn_weight_grad_scratch_floats(rows, Hq)
    for Hq in (32, 96):
        assert lib.ic3_rnn_backward_wide_supported(env._h, Hq) == 0 and lib.ic3_mlp_backward_wide_supported(env._h, Hq) == 0
        assert lib.ic3_rnn_backward_wide_partials(R, Hq) == 0 and lib.ic3_mlp_backward_wide_partials(R, Hq) == 0
        assert lib.ic3_rnn_weight_grad_wide_scratch_floats(R, Hq) == 0
    assert lib.ic3_rnn_backward_supported(env._h, 256) == 0 and lib.ic3_mlp_backward_supported(env._h, 256) == 0
    assert lib.ic3_rnn_backward_partials(R, 256) == 0 and lib.ic3_mlp_backward_partials(R, 256) == 0
    assert lib.ic3_rnn_weight_grad_scratch_floats(R, 256) == 0
    f = np.zeros((R, 256), np.float32)
    d = np.zeros((R, 6), np.float32)
    assert lib.ic3_rnn_weight_grad_wide(p(f), p(f), None, R, 96, p(f), 0, p(f), None) == -38
    assert lib.ic3_rnn_weight_grad(p(f), p(f), None, R, 256, p(f), 0, p(f), None) == -38
    assert lib.ic3_rnn_tanh_backward_step_wide(None, p(f), p(d), p(f), 6, p(f), None, p(f), p(f), p(f), 0, R, 96, None) == -38
    assert lib.ic3_rnn_tanh_backward_step(None, p(f), p(d), p(f), 6, p(f), None, p(f), p(f), p(f), 0, R, 256, None) == -38
    assert lib.ic3_mlp_backward_step_wide(p(f), p(f), p(d), p(f), 6, p(f), p(f), p(f), p(f), 0, R, 96, None) == -38
    assert lib.ic3_mlp_backward_step(p(f), p(f), p(d), p(f), 6, p(f), p(f), p(f), p(f), 0, R, 256, None) == -38
    rb, mb = binding.RnnBptt(), binding.MlpBptt()
    rb.struct_size, mb.struct_size = C.sizeof(rb) - 8, C.sizeof(mb) - 8
    assert lib.ic3_rnn_backward_wide(env._h, C.byref(rb), None) == -22 and b"ic3_rnn_bptt has" in lib.ic3_last_error()
    assert lib.ic3_mlp_backward_wide(env._h, C.byref(mb), None) == -22 and b"ic3_mlp_bptt has" in lib.ic3_last_error()
    rb.struct_size, mb.struct_size = C.sizeof(rb), C.sizeof(mb)
    rb.T, rb.E, rb.N, rb.H, rb.OT = 1, env.E, env.N, 96, 6
    mb.T, mb.E, mb.N, mb.H, mb.OT = 1, env.E, env.N, 96, 6
    assert lib.ic3_rnn_backward_wide(env._h, C.byref(rb), None) == -38 and b"64 / 128 / 256" in lib.ic3_last_error()
    assert lib.ic3_mlp_backward_wide(env._h, C.byref(mb), None) == -38 and b"64 / 128 / 256" in lib.ic3_last_error()
    env.close()

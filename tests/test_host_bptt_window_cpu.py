"""CPU: ic3_bptt_backward — the LSTM window backward as ONE host call — on the host build of the product's own sources
(tests/host/libic3rollout_host.so) against the float64 window backward of tests/bptt_window_ref.py: which steps are detached, which
row factors go where, the two chains' offsets into every buffer, NULL mask entries, the ring and the one-buffer form of dxh,
enc_first; then ic3_lstm_weight_grad on the record the call left; and what the call refuses before its first launch."""
import ctypes as C

import numpy as np
import pytest

import bptt_window_ref as ref
from host_abi_util import HostEnv, check, host_lib, p


def _env(kind, E):
    if kind == 'pp':
        return HostEnv.pp(3, 6, 1, 'mixed', E, seed=3)
    return HostEnv.tj(5, 6, 1, 'easy', E, seed=3, add_rate_min=0.6, add_rate_max=0.6)


class _Window(object):
    """The buffers of one call: written ones NaN-filled, added-to ones pre-filled with known non-zero values."""

    def __init__(self, lib, env, w, ring, two_chains, work):
        from ic3net_amd import _lib as binding
        T, E, N, H, OT = w['T'], w['E'], w['N'], w['H'], w['OT']
        R = E * N
        self.w, self.ring = w, ring
        self.gates, self.dh, self.dc = w['gates'].copy(), w['dh'].copy(), w['dc'].copy()
        self.dxh = np.full((T, R, 2 * H) if ring else (R, 2 * H), np.nan, np.float32)
        rng = np.random.default_rng(99)
        self.bias0 = rng.standard_normal(((R + 63) // 64, 4 * H)).astype(np.float32)
        E1 = lib.ic3_bptt_first_chain_envs(E, N) if (two_chains and ring) else E
        self.slots = lib.ic3_comm_backward_partials(E1, N) + (lib.ic3_comm_backward_partials(E - E1, N) if E1 < E else 0)
        self.dcw0 = rng.standard_normal((self.slots, H, H)).astype(np.float32)
        self.bias, self.dcw = self.bias0.copy(), self.dcw0.copy()
        self.wb3 = np.zeros(3 * 4 * H * 2 * H, np.uint16)
        check(lib.ic3_policy_pack_split_bwd(p(w['w_ih']), p(w['w_hh']), p(self.wb3), H, None))
        b = binding.Bptt()
        b.struct_size = C.sizeof(b)
        b.T, b.E, b.N, b.H, b.OT = T, E, N, H, OT
        b.gates, b.hs, b.cs, b.dhead = self.gates.ctypes.data, w['hs'].ctypes.data, w['cs'].ctypes.data, w['dhead'].ctypes.data
        self._keep = []
        for name in ('alive', 'gate'):
            if w[name] is not None:
                arr = (C.c_void_p * T)(*[None if m is None else m.ctypes.data for m in w[name]])
                self._keep.append(arr)
                setattr(b, name, C.cast(arr, C.POINTER(C.c_void_p)))
        b.row_live = w['row_live'].ctypes.data if w['row_live'] is not None else None
        b.row_keep = w['row_keep'].ctypes.data if w['row_keep'] is not None else None
        b.lstm_wp3_bwd, b.w_heads, b.c_weight = self.wb3.ctypes.data, w['w_heads'].ctypes.data, w['c_weight'].ctypes.data
        b.dh, b.dc, b.dxh = self.dh.ctypes.data, self.dc.ctypes.data, self.dxh.ctypes.data
        b.dbias_partials, b.dcw_partials, b.enc_work = self.bias.ctypes.data, self.dcw.ctypes.data, work.ctypes.data
        b.dxh_step = R * 2 * H if ring else 0
        b.two_chains = int(two_chains)
        self.b = b


CASES = {
    # A: lock-step at hid 64, E = 130 -> the ring with two chains splits at E1 = 64 (192 rows | 198 rows: a ragged last tile in the
    #    second chain), hard-attention gate masks, alive NULL; T = 4 with detach_gap = 2 detaches the window's last step
    'A-T4-gap2': dict(kind='pp', E=130, H=64, T=4, gap=2, ring=True, two=True),
    'A-T5-gap3': dict(kind='pp', E=130, H=64, T=5, gap=3, ring=True, two=True),
    # B: collection mode on Traffic-Junction, alive[0] NULL and later entries set, the one-buffer form (per-step encoder accumulate),
    #    a second window with enc_first = 0 that adds;  B2: collection mode through the ring and two chains
    'B-collect-one-buffer': dict(kind='tj', E=30, H=64, T=4, collect=True, alive='first_null', ring=False, two=False, second=True),
    'B2-collect-ring-two-chains': dict(kind='pp', E=130, H=64, T=3, collect=True, alive='all', ring=True, two=True),
    'C-comm-zero': dict(kind='pp', E=130, H=64, T=3, gap=2, ring=True, two=True, comm_zero=True),
    'D-sum-mode': dict(kind='tj', E=30, H=64, T=3, gap=0, alive='all', ring=False, two=False, avg=False),
    'E-hid128-one-tile': dict(kind='pp', E=20, H=128, T=2, gap=0, ring=True, two=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_window_backward_against_float64(name):
    """dgates of every step, the dxh ring (the last-written step in the one-buffer form), dh / dc leaving the window, EVERY row of the
    bias partials (their sum would hide a wrong chain offset), the sum over the dcw slots (and their count against the two chains'
    grids), the encoder's dWt / db through the finish that goes with the form, and the LSTM weight gradient of the in-place record —
    each against the float64 window backward at its bar (bptt_window_ref.check)."""
    from test_host_abi_cpu import _play
    lib = host_lib()
    cfg = CASES[name]
    env = _env(cfg['kind'], cfg['E'])
    T, H, OT = cfg['T'], cfg['H'], 6
    E, N = env.E, env.N
    R = E * N
    ring, two = cfg['ring'], cfg['two']
    gap, avg, comm_zero = cfg.get('gap', 0), cfg.get('avg', True), cfg.get('comm_zero', False)
    w = ref.make_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False), alive=cfg.get('alive', 'none'))
    snaps, obs = [], []
    for t in range(T):
        _play(env, 2 + t, 70 + t)
        snaps.append(env.snapshot())
        obs.append(env.observe().reshape(R, env.obs_dim).astype(np.float64))
    snaps = np.ascontiguousarray(np.stack(snaps))
    want = ref.reference_of(w, obs=obs, detach_gap=gap, mode_avg=avg, comm_zero=comm_zero)
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H) if ring else lib.ic3_env_encode_backward_work(env._h, H))
    assert n > 0
    work = np.full((n,), np.nan, np.float32)
    E1 = lib.ic3_bptt_first_chain_envs(E, N)
    if two:
        assert (E1 < E) == (E >= 128) and (E1 == E or (E1 * N) % 64 == 0)
    windows = 2 if cfg.get('second') else 1
    for k in range(windows):
        win = _Window(lib, env, w, ring, two, work)
        b = win.b
        b.mode_avg, b.comm_zero, b.detach_gap, b.enc_first = int(avg), int(comm_zero), gap, int(k == 0)
        b.snaps, b.snap_words = snaps.ctypes.data, snaps.shape[1]
        if k:                                                    # the second window adds onto what the first left
            win.bias[:], win.dcw[:] = bias_left, dcw_left
        check(lib.ic3_bptt_backward(env._h, C.byref(b), None))
        bias_left, dcw_left = win.bias.copy(), win.dcw.copy()
    errs = dict(dgates=ref.rel_err(win.gates, want['dgates']), dh=ref.rel_err(win.dh, want['dh']), dc=ref.rel_err(win.dc, want['dc']))
    errs['dxh'] = ref.rel_err(win.dxh, want['dxh']) if ring else ref.rel_err(win.dxh, want['dxh'][0])
    errs['dbias_rows'] = ref.rel_err(win.bias, win.bias0.astype(np.float64) + windows * want['dbias_rows'])
    if comm_zero:
        np.testing.assert_array_equal(win.dcw, win.dcw0)         # (nothing of C is touched)
    else:
        from ic3net_amd import _lib as binding                   # (the count the Python binding sizes the buffer by)
        assert win.slots == lib.ic3_comm_backward_partials(E1 if (two and ring) else E, N) + \
            (lib.ic3_comm_backward_partials(E - E1, N) if (two and ring and E1 < E) else 0)
        errs['dcw'] = ref.rel_err(win.dcw.astype(np.float64).sum(0), win.dcw0.astype(np.float64).sum(0) + windows * want['dcw'])
    dwt = np.full((env.obs_dim, H), np.nan, np.float32)
    db = np.full((H,), np.nan, np.float32)
    fin = lib.ic3_env_encode_backward_window_finish if ring else lib.ic3_env_encode_backward_finish
    check(fin(env._h, H, p(dwt), p(db), p(work), None))
    errs['enc_dwt'] = ref.rel_err(dwt, windows * want['enc_dwt'])
    errs['enc_db'] = ref.rel_err(db, windows * want['enc_db'])
    # the weight gradient of the record the call left in place: [inp | live hs]^T . dgates, added onto what dW held
    Q = T * R
    dW0 = np.random.default_rng(5).standard_normal((2 * H, 4 * H)).astype(np.float32)
    dW = dW0.copy()
    scratch = np.zeros(lib.ic3_lstm_weight_grad_scratch_floats(Q, H), np.float32)
    check(lib.ic3_lstm_weight_grad(p(w['inp']), H, p(w['hs']), p(win.gates), p(w['row_live']), Q, H, p(dW), 1, 1, p(scratch), None))
    errs['dW'] = ref.rel_err(dW, dW0.astype(np.float64) + want['dW'])
    env.close()
    ref.check('host/' + name, errs)


def test_dcw_slot_count_matches_the_binding():
    """ops.bptt_dcw_partials' arithmetic (two chains: the first chain's grid + the second's) on the host library's answers."""
    lib = host_lib()
    for E, N in ((130, 3), (3100, 20), (200, 3), (64, 10), (127, 5)):
        E1 = lib.ic3_bptt_first_chain_envs(E, N)
        assert E1 == (E if E < 128 else (E // 2) & ~63)
        ept = 64 // N
        grid = lambda e: (lambda tiles: (tiles + (tiles + 511) // 512 - 1) // ((tiles + 511) // 512))((e + ept - 1) // ept)
        assert lib.ic3_comm_backward_partials(E1, N) == grid(E1)
        if E1 < E:
            assert lib.ic3_comm_backward_partials(E - E1, N) == grid(E - E1)
    assert lib.ic3_comm_backward_partials(1536, 20) + lib.ic3_comm_backward_partials(1564, 20) == 512 + 261


def _refusal_window(lib, env, **kw):
    w = ref.make_window(1, 3, env.E, env.N, 64, 6, collect=kw.pop('collect', False))
    n = int(lib.ic3_env_encode_backward_window_work(env._h, 64))
    work = np.zeros((n,), np.float32)
    win = _Window(lib, env, w, True, True, work)
    snaps = np.ascontiguousarray(np.stack([env.snapshot()] * 3))
    win.b.snaps, win.b.snap_words = snaps.ctypes.data, snaps.shape[1]
    win.snaps, win.work = snaps, work                            # (kept alive: the descriptor holds raw addresses)
    win.b.mode_avg, win.b.enc_first = 1, 1
    return win


def test_detach_gap_with_row_keep_is_refused_before_the_first_launch():
    """detach_gap > 0 together with row_keep: -EINVAL and a reason, with the record, dh / dc, the partials and the ring as they were
    (the gate launch of the first detached step would refuse it — after later steps' gates were overwritten)."""
    lib = host_lib()
    env = _env('pp', 130)
    env.reset(0)
    win = _refusal_window(lib, env, collect=True)
    win.b.detach_gap = 2
    assert lib.ic3_bptt_backward(env._h, C.byref(win.b), None) == -22
    msg = lib.ic3_last_error()
    assert b"detach_gap" in msg and b"row_keep" in msg
    np.testing.assert_array_equal(win.gates, win.w['gates'])
    np.testing.assert_array_equal(win.dh, win.w['dh'])
    np.testing.assert_array_equal(win.dc, win.w['dc'])
    np.testing.assert_array_equal(win.bias, win.bias0)
    np.testing.assert_array_equal(win.dcw, win.dcw0)
    assert np.isnan(win.dxh).all()
    win.b.detach_gap = 0                                         # (the same descriptor without the gap runs)
    check(lib.ic3_bptt_backward(env._h, C.byref(win.b), None))
    assert np.isfinite(win.gates).all() and not np.array_equal(win.gates, win.w['gates'])
    env.close()

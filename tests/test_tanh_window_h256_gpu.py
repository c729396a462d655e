"""GPU: the tanh-recurrence and the IC baseline's window backwards at hid 256 (ops.rnn_backward / ops.mlp_backward /
ops.rnn_weight_grad through the _wide entries: rnn_tanh_bwd_kernel<256>, mlp_bwd_kernel<256>, rnn_wgrad_kernel<256>) against the
float64 window backwards of tests/tanh_window_ref.py on the shapes of tests/test_tanh_window_gpu.py, each quantity at its bar from
tests/tanh_window_h256_bars.py, every case launched a second time on fresh copies: bit-identical.  Then the two baselines end to
end at hid 256: the update takes the window path and agrees with the per-step loop on the same record."""
import numpy as np
import pytest
import torch

import tanh_window_ref as ref
from tanh_window_h256_bars import check as check_bars
from test_tanh_window_gpu import _launch_mlp, _launch_rnn, _num, _pp, _record_states, _tj

pytestmark = pytest.mark.gpu

H = 256

# one workgroup slot per CU at hid 256: up to 256 tiles one partial per 64-row tile
RNN_CASES = {
    # R = 1310 = 20 tiles + 30 rows; detach points inside the window (steps 1 and 3); the last step's h_t in a buffer of its own
    'rnn-h256-pp-hard-E131-T5-gap2-h-last': dict(env=lambda: _pp(10, 20, 1, 131), T=5, gap=2, h_last='separate'),
    # row_keep[t - 1] / row_live[t]; the per-step encoder form; T + 1 slots; the widest heads
    'rnn-h256-tj-easy-E130-T4-collect-per-step-OT16': dict(env=lambda: _tj(5, 6, 'easy', 130), T=4, collect=True, enc_window=False, OT=16),
    # two windows of 3 steps on one set of accumulators, the later one first (the second: enc_first off, the dh the first left)
    'rnn-h256-tj-hard-E67-two-windows-T3-collect': dict(env=lambda: _tj(20, 18, 'hard', 67), T=6, collect=True, windows=((3, 3), (0, 3))),
    # R = 17100 rows = 267 tiles + 12 rows on 256 slots: 134 workgroups x 2 tiles, the ragged tile the last workgroup's second
    'rnn-h256-pp-n3-E5700-T2-two-tiles-a-workgroup': dict(env=lambda: _pp(3, 6, 1, 5700), T=2, walk=True),
    # a one-step window that is all detach; the single-column heads; no weight gradient
    'rnn-h256-pp-n3-E9-T1-gap1-OT1-no-a2': dict(env=lambda: _pp(3, 6, 1, 9), T=1, gap=1, OT=1, a2=False),
}


def _walk_ok(partials, rows):
    """a workgroup walks at least 2 tiles, and the ragged last tile is not a workgroup's first"""
    tiles = (rows + 63) // 64
    return rows % 64 != 0 and partials < tiles and tiles - 1 >= partials


@pytest.mark.parametrize("name", list(RNN_CASES))
def test_rnn_window_backward_h256_against_float64(name):
    """Every slot of the dz ring, dh leaving the window, the partials' column sum on top of their pre-fill (and every partial row
    where there is one per tile), a2_grad on top of its pre-fill, the encoder's dWt / db through the finish that goes with the
    form; then the same call(s) again on fresh copies: dz, dh, the partials and a2_grad the same bits."""
    from ic3net_amd import ops
    cfg = RNN_CASES[name]
    env = cfg['env']()
    T, OT = cfg['T'], cfg.get('OT', 6)
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.rnn_backward_supported(env, H)
    if cfg.get('walk'):
        assert _walk_ok(ops.rnn_backward_partials(R, H), R)
    else:
        assert ops.rnn_backward_partials(R, H) == (R + 63) // 64
    w = ref.make_rnn_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False), h_last=cfg.get('h_last', 'slot'))
    snaps, obs = _record_states(env, T)
    want = ref.rnn_reference_of(w, obs=obs, detach_gap=cfg.get('gap', 0))
    got = _launch_rnn(env, w, cfg, snaps)
    errs = ref.rnn_errors(want, _num(got['dz']), _num(got['dh']), _num(got['parts']), _num(got['parts0']),
                          _num(got['a2g']) if cfg.get('a2', True) else None, _num(got['a2g0']))
    assert ('dbias_tiles' in errs) == (not cfg.get('walk'))
    if not cfg.get('a2', True):
        assert torch.equal(got['a2g'].cpu(), got['a2g0'])
    dwt, db = env.encode_backward_window_finish(H) if cfg.get('enc_window', True) else env.encode_backward_finish(H)
    errs['enc_dwt'], errs['enc_db'] = ref.rel_err(_num(dwt), want['enc_dwt']), ref.rel_err(_num(db), want['enc_db'])
    again = _launch_rnn(env, w, cfg, snaps)
    for k in ('dz', 'dh', 'parts', 'a2g'):
        assert torch.equal(got[k], again[k]), k
    check_bars('gpu/' + name, errs)


MLP_CASES = {
    # Q = 3 x 1310 rows: tiles that span two steps' rows, a ragged last one; the table form of the encoder; both finishes
    'mlp-h256-pp-hard-E131-T3-table': dict(env=lambda: _pp(10, 20, 1, 131), T=3, table=True),
    # Q = 3 x 5466 = 16398 rows = 256 tiles + 14 rows on 256 slots: 129 workgroups, the next-tile prefetch, the ragged tile a second one
    'mlp-h256-pp-n3-E1822-T3-two-tiles-a-workgroup': dict(env=lambda: _pp(3, 6, 1, 1822), T=3, walk=True),
}


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_window_backward_h256_against_float64(name):
    """The x1 / dz / de rings, the partials from a NaN pre-fill (their column sum; every row where there is one per tile), a2_grad
    on top of its pre-fill, the encoder's dWt / db through the ordered and the plain finish; then the same call again on fresh
    copies: the rings, the partials and a2_grad the same bits."""
    from ic3net_amd import ops
    cfg = MLP_CASES[name]
    env = cfg['env']()
    T, OT = cfg['T'], cfg.get('OT', 6)
    E, N = env.nenvs, env.nagents_env
    Q = T * E * N
    assert ops.mlp_backward_supported(env, H)
    if cfg.get('walk'):
        assert _walk_ok(ops.mlp_backward_partials(Q, H), Q)
    else:
        assert ops.mlp_backward_partials(Q, H) == (Q + 63) // 64
    w = ref.make_mlp_window(sum(map(ord, name)), T, E, N, H, OT, env.obs_dim)
    snaps, obs = _record_states(env, T)
    want = ref.mlp_reference_of(w, obs)
    got = _launch_mlp(env, w, cfg, snaps)
    errs = ref.mlp_errors(want, _num(got['x1']), _num(got['dz']), _num(got['de']), _num(got['parts']), _num(got['a2g']),
                          _num(got['a2g0']))
    assert ('dbias_tiles' in errs) == (not cfg.get('walk'))
    for tag, fin in (('_ordered', env.encode_backward_window_finish_ordered), ('', env.encode_backward_window_finish)):
        dwt, db = fin(H)
        errs['enc_dwt' + tag] = ref.rel_err(_num(dwt), want['enc_dwt'])
        errs['enc_db' + tag] = ref.rel_err(_num(db), want['enc_db'])
    again = _launch_mlp(env, w, cfg, snaps)
    for k in ('x1', 'dz', 'de', 'parts', 'a2g'):
        assert torch.equal(got[k], again[k]), k
    check_bars('gpu/' + name, errs)


def test_rnn_weight_grad_h256_ragged_rows_row_live_accumulate():
    """ops.rnn_weight_grad at hid 256 on Q = 100003 rows (no multiple of 16, nor of the K slices) with row_live: accumulate off over
    a NaN dA2, then on: twice the product; the same two calls again: the same bits."""
    from ic3net_amd import ops
    Q = 100003
    rng = np.random.default_rng(5)
    dz = rng.standard_normal((Q, H)).astype(np.float32)
    h = np.tanh(rng.standard_normal((Q, H))).astype(np.float32)
    live = (rng.random(Q) < 0.8).astype(np.float32)
    want = dz.astype(np.float64).T @ (h.astype(np.float64) * live[:, None])
    dzd, hd, lived = (torch.from_numpy(a).cuda() for a in (dz, h, live))

    def run():
        dA = torch.full((H, H), float('nan'), device='cuda')
        ops.rnn_weight_grad(dzd, hd, dA, row_live=lived, accumulate=False)
        first = dA.clone()
        ops.rnn_weight_grad(dzd, hd, dA, row_live=lived, accumulate=True)
        torch.cuda.synchronize()
        return first, dA
    first, both = run()
    assert torch.equal(both, first + first)
    again = run()
    assert torch.equal(first, again[0]) and torch.equal(both, again[1])
    check_bars('gpu/wgrad-h256-Q100003-row-live', dict(a2_grad=ref.rel_err(_num(first), want),
                                                      a2_grad_accumulated=ref.rel_err(_num(both), 2 * want)))


@pytest.mark.parametrize("collect", [False, True])
def test_iric_tanh_h256_update_takes_the_window_and_equals_the_loop(monkeypatch, collect):
    """pp_hard_iric_tanh at hid 256, E = 64, T = 8: the update runs bptt._backward_window_rnn (lock-step with detach points inside the
    window; collection mode over two windows with the carry between them) and agrees with the per-step loop on the same record."""
    from test_rnn_backward_gpu import _agree, _grads, _paths, _recorded
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_iric_tanh', 64, 8, collect=collect, hid_size=H)
    assert len(recs) == (2 if collect else 1)
    g1 = _grads(tr, batch, recs, True)
    assert seen == ['_backward_window_rnn'] * len(recs)
    del seen[:]
    g0 = _grads(tr, batch, recs, False)
    assert seen == ['_backward_episode_baseline'] * len(recs)
    _agree(g1, g0)


def test_ic_h256_update_takes_the_window_and_equals_the_loop(monkeypatch):
    """pp_hard_ic at hid 256, E = 64, T = 8: the rollout records h of every step, the update runs bptt._backward_window_mlp and
    agrees with the per-step loop on the same record, which it leaves as it was."""
    from test_mlp_backward_gpu import LOOP, WINDOW, _paths
    from test_rnn_backward_gpu import _agree, _grads, _recorded
    seen = _paths(monkeypatch)
    tr, a, batch, recs = _recorded('pp_hard_ic', 64, 8, hid_size=H)
    assert len(recs) == 1 and recs[0].h_fin is not None and recs[0].h_fin_n == recs[0].n
    h_fin = recs[0].h_fin.clone()
    g1 = _grads(tr, batch, recs, True)
    assert seen == WINDOW
    del seen[:]
    g0 = _grads(tr, batch, recs, False)
    assert seen == LOOP
    _agree(g1, g0)
    assert torch.equal(recs[0].h_fin, h_fin)

"""GPU: ops.rnn_backward(walk=True) — ic3_rnn_backward_wide on an ic3_rnn_bptt_walk descriptor, the tanh recurrence's window backward
with its T steps walked in ONE launch (rnn_tanh_bwd_walk_kernel<64 / 128 / 256>) — against the per-step call on the same inputs, on
the case shapes of tests/test_tanh_window_gpu.py plus one of tests/test_tanh_window_h256_gpu.py, zeroed partials and a2_grad:
  one tile per workgroup: the dz ring, dh leaving the window, EVERY partial row, a2_grad and the encoder's dWt / db through the
  window form's ordered finish bit for bit (the per-step encoder form finishes with float atomics: that case's dWt / db are held to
  the float64 window backward at the per-step call's bars of tests/tanh_window_bars.py);
  the two `two-tiles-a-workgroup` shapes (the per-step call has fewer partial rows than there are tiles): dz, dh and a2_grad bit for
  bit, the partials as column sums against the float64 window backward of tests/tanh_window_ref.py at the bar of
  tests/tanh_walk_bars.py (4 x the per-step call's own figure on these inputs, never above 1e-5).
Every case is launched a second time on fresh copies: bit-identical."""
import pytest
import torch

import tanh_window_ref as ref
from test_tanh_window_gpu import RNN_CASES, _num, _record_states, _up
from test_tanh_window_h256_gpu import RNN_CASES as RNN_CASES_256

pytestmark = pytest.mark.gpu

CASES = dict(RNN_CASES)
CASES['rnn-h256-pp-hard-E131-T5-gap2-h-last'] = dict(RNN_CASES_256['rnn-h256-pp-hard-E131-T5-gap2-h-last'], H=256)


def _launch(env, w, cfg, snaps, walk):
    """The case's window(s) on fresh device copies through the per-step call (walk = False) or the walk"""
    from ic3net_amd import ops
    dev = env.device
    T, E, N, H = w['T'], w['E'], w['N'], w['H']
    R = E * N
    nparts = (R + 63) // 64 if walk else ops.rnn_backward_partials(R, H)
    parts, a2g, dh = torch.zeros((nparts, H), device=dev), torch.zeros((H, H), device=dev), _up(w['dh'], dev)
    dz = torch.full((T, R, H), float('nan'), device=dev)
    hs, dhead, h_last = _up(w['hs'], dev), _up(w['dhead'], dev), _up(w['h_last'], dev)
    live, keep = _up(w['row_live'], dev), _up(w['row_keep'], dev)
    a2, w_heads = _up(w['a2'], dev), _up(w['w_heads'], dev)
    for k, (t0, n) in enumerate(cfg.get('windows', ((0, T),))):
        if k and keep is not None:                               # (the caller's part: what crosses the border between two windows)
            dh.mul_(keep[t0 + n - 1].unsqueeze(1))
        ops.rnn_backward(env, n, E, N, H, hs[t0:], dhead[t0:t0 + n], snaps[t0:t0 + n], a2, w_heads, dh, dz[t0:t0 + n], parts,
                         h_last=h_last if t0 + n == T else None, detach_gap=cfg.get('gap', 0),
                         row_live=None if live is None else live[t0:t0 + n], row_keep=None if keep is None else keep[t0:t0 + n],
                         enc_first=(k == 0), enc_window=cfg.get('enc_window', True), a2_grad=a2g if cfg.get('a2', True) else None,
                         walk=walk)
    torch.cuda.synchronize()
    return dict(dz=dz, dh=dh, parts=parts, a2g=a2g)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_walk_against_the_per_step_call(name):
    from ic3net_amd import ops
    from tanh_walk_bars import BARS, CAP
    cfg = CASES[name]
    env = cfg['env']()
    T, H, OT = cfg['T'], cfg['H'], cfg.get('OT', 6)
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.rnn_backward_supported(env, H)
    one_tile_each = ops.rnn_backward_partials(R, H) == (R + 63) // 64
    assert one_tile_each == (not cfg.get('walk'))                # ('walk' in those tables: a workgroup owns more than one tile)
    w = ref.make_rnn_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False), h_last=cfg.get('h_last', 'slot'))
    snaps, obs = _record_states(env, T)
    window_form = cfg.get('enc_window', True)
    # (the window form's ordered finish is identical run to run; the per-step form's adds with float atomics)
    enc_fin = env.encode_backward_window_finish_ordered if window_form else env.encode_backward_finish
    steps = _launch(env, w, cfg, snaps, walk=False)
    steps_enc = [v.clone() for v in enc_fin(H)]
    walk = _launch(env, w, cfg, snaps, walk=True)
    walk_enc = [v.clone() for v in enc_fin(H)]
    assert not torch.isnan(walk['dz']).any()
    for k in ('dz', 'dh', 'a2g') + (('parts',) if one_tile_each else ()):
        assert _same_bits(steps[k], walk[k]), k
    if window_form:                                              # (the encoder's stage reads the ring alone)
        for k, a, b in zip(('enc_dwt', 'enc_db'), steps_enc, walk_enc):
            assert _same_bits(a, b), k
    else:                                                        # float atomics: against float64, at the per-step call's own bars
        from tanh_window_bars import BARS as STEP_BARS
        want = ref.rnn_reference_of(w, obs=obs, detach_gap=cfg.get('gap', 0))
        for k, got in zip(('enc_dwt', 'enc_db'), walk_enc):
            err = ref.rel_err(_num(got), want[k])
            print("tanh-walk gpu/%s %s %.3e" % (name, k, err))
            assert err <= STEP_BARS['gpu/' + name][k], (k, err)
    if not cfg.get('a2', True):
        assert not walk['a2g'].any()
    if not one_tile_each:
        want = ref.rnn_reference_of(w, detach_gap=cfg.get('gap', 0))['dbias_cols']
        err_steps = ref.rel_err(_num(steps['parts']).sum(0), want)
        err_walk = ref.rel_err(_num(walk['parts']).sum(0), want)
        print("tanh-walk gpu/%s dbias_cols: per-step call %.3e, walk %.3e" % (name, err_steps, err_walk))
        bar = BARS['gpu/' + name]['dbias_cols']
        assert bar <= CAP and err_walk <= bar, (err_walk, bar)
    again = _launch(env, w, cfg, snaps, walk=True)
    for k in ('dz', 'dh', 'parts', 'a2g'):
        assert _same_bits(walk[k], again[k]), k

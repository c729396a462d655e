"""GPU: ic3_rnn_backward (ops.rnn_backward) and ic3_mlp_backward (ops.mlp_backward) — the tanh-recurrence and the IC baseline's
window backwards as ONE host call each — against the float64 window backwards of tests/tanh_window_ref.py on synthetic records:
the slot a step's h_t comes from (and the h_last buffer), the step whose row_keep scales what crosses, the detach points, dh in
place over the steps, partials and a2_grad added to over steps and windows, both encoder forms, a second window with enc_first
off, launches whose workgroups walk more than one tile; the IC call's three rings, its table encoder and both finishes.  Every case
is launched a second time on fresh copies: bit-identical."""
import numpy as np
import pytest
import torch

import tanh_window_ref as ref

pytestmark = pytest.mark.gpu


def _pp(N, dim, vision, E):
    from test_env_parity_gpu import make_pp
    return make_pp(N, dim, vision, 'mixed', E, seed=3)


def _tj(N, dim, difficulty, E):
    from test_env_parity_gpu import make_tj
    return make_tj(N, dim, 1, difficulty, E, seed=3, add_rate_min=0.5, add_rate_max=0.5)


def _record_states(env, T):
    """T snapshots of random play, two steps apart, and the dense observation of each on the CPU in float64"""
    E, N = env.nenvs, env.nagents_env
    rng = np.random.default_rng(7)
    env.reset()
    snaps = torch.empty((T, env.dims.state_words), dtype=torch.int32, device=env.device)
    obs = []
    for t in range(T):
        for _ in range(2):
            env.step(rng.integers(0, env.dims.naction, (E, N)), observe=False)
        env.snapshot(out=snaps[t])
        obs.append(env.observe().reshape(E * N, env.obs_dim).cpu().double().numpy())
    return snaps, obs


def _up(a, dev):
    return None if a is None else torch.from_numpy(a).to(dev)


def _num(v):
    return v.double().cpu().numpy()


# 256 CUs: 256 workgroup slots at hid 128, 512 at hid 64 — up to there one partial per 64-row tile
RNN_CASES = {
    # R = 1310 = 20 tiles + 30 rows; detach points inside the window (steps 1 and 3); the last step's h_t in a buffer of its own
    'rnn-h128-pp-hard-E131-T5-gap2-h-last': dict(env=lambda: _pp(10, 20, 1, 131), H=128, T=5, gap=2, h_last='separate'),
    # row_keep[t - 1] / row_live[t]; the per-step encoder form; T + 1 slots; the widest heads
    'rnn-h64-tj-easy-E130-T4-collect-per-step-OT16': dict(env=lambda: _tj(5, 6, 'easy', 130), H=64, T=4, collect=True, enc_window=False,
                                                          OT=16),
    # two windows of 3 steps on one set of accumulators, the later one first: the second call runs with enc_first off, takes the
    # dh the first left (times the border's row_keep: the caller's part) and adds onto the same partials and a2_grad; the
    # reference runs over all 6 steps once
    'rnn-h128-tj-hard-E67-two-windows-T3-collect': dict(env=lambda: _tj(20, 18, 'hard', 67), H=128, T=6, collect=True,
                                                        windows=((3, 3), (0, 3))),
    # R = 17100 rows = 268 tiles on 256 slots: 134 workgroups x 2 tiles
    'rnn-h128-pp-n3-E5700-T2-two-tiles-a-workgroup': dict(env=lambda: _pp(3, 6, 1, 5700), H=128, T=2, walk=True),
    # R = 32800 rows = 513 tiles on 512 slots: 257 workgroups, all but one with 2 tiles
    'rnn-h64-tj-easy-E6560-T2-collect-two-tiles-a-workgroup': dict(env=lambda: _tj(5, 6, 'easy', 6560), H=64, T=2, collect=True, walk=True),
    # a one-step window that is all detach; the single-column heads; no weight gradient
    'rnn-h64-pp-n3-E9-T1-gap1-OT1-no-a2': dict(env=lambda: _pp(3, 6, 1, 9), H=64, T=1, gap=1, OT=1, a2=False),
}


def _launch_rnn(env, w, cfg, snaps):
    """The case's ic3_rnn_backward call(s) on fresh device copies; returns the buffers written (NaN-filled) / added to (pre-filled
    with known values)."""
    from ic3net_amd import ops
    dev = env.device
    T, E, N, H = w['T'], w['E'], w['N'], w['H']
    R = E * N
    g = torch.Generator().manual_seed(99)
    parts0 = torch.randn((ops.rnn_backward_partials(R, H), H), generator=g)
    a2g0 = torch.randn((H, H), generator=g)
    parts, a2g, dh = parts0.to(dev), a2g0.to(dev), _up(w['dh'], dev)
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
                         enc_first=(k == 0), enc_window=cfg.get('enc_window', True), a2_grad=a2g if cfg.get('a2', True) else None)
    torch.cuda.synchronize()
    return dict(dz=dz, dh=dh, parts=parts, a2g=a2g, parts0=parts0, a2g0=a2g0)


@pytest.mark.parametrize("name", list(RNN_CASES))
def test_rnn_window_backward_against_float64(name):
    """Every slot of the dz ring, dh leaving the window, the partials' column sum on top of their pre-fill (and every partial row
    where there is one per tile), a2_grad on top of its pre-fill, the encoder's dWt / db through the finish that goes with the form
    — against the float64 window backward, each at its bar (tanh_window_ref.check); then the same call(s) again on fresh copies:
    dz, dh, the partials and a2_grad the same bits."""
    from ic3net_amd import ops
    cfg = RNN_CASES[name]
    env = cfg['env']()
    T, H, OT = cfg['T'], cfg['H'], cfg.get('OT', 6)
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.rnn_backward_supported(env, H)
    tiles = (R + 63) // 64
    if cfg.get('walk'):
        assert ops.rnn_backward_partials(R, H) < tiles           # (a workgroup walks more than one tile)
    else:
        assert ops.rnn_backward_partials(R, H) == tiles
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
    ref.check('gpu/' + name, errs)


MLP_CASES = {
    # Q = 3 x 1310 rows: tiles that span two steps' rows, a ragged last one; the table form of the encoder; both finishes
    'mlp-h128-pp-hard-E131-T3-table': dict(env=lambda: _pp(10, 20, 1, 131), H=128, T=3, table=True),
    'mlp-h64-tj-easy-E130-T4-per-step-OT16': dict(env=lambda: _tj(5, 6, 'easy', 130), H=64, T=4, enc_window=False, OT=16),
    # Q = 3 x 5466 = 16398 rows = 257 tiles on 256 slots: the next-tile prefetch inside one window call
    'mlp-h128-pp-n3-E1822-T3-two-tiles-a-workgroup': dict(env=lambda: _pp(3, 6, 1, 1822), H=128, T=3, walk=True),
    # the same window twice on one a2_grad and one set of encoder sums, the second time with enc_first off
    'mlp-h64-tj-easy-E40-T2-table-two-windows': dict(env=lambda: _tj(5, 6, 'easy', 40), H=64, T=2, table=True, windows=2),
}


def _launch_mlp(env, w, cfg, snaps):
    """The case's ic3_mlp_backward call(s) on fresh device copies; returns the buffers written (NaN-filled) / added to."""
    from ic3net_amd import ops
    dev = env.device
    T, E, N, H = w['T'], w['E'], w['N'], w['H']
    R = E * N
    a2g0 = torch.randn((H, H), generator=torch.Generator().manual_seed(99))
    a2g = a2g0.to(dev)
    h, dhead, a2, w_heads = _up(w['h'], dev), _up(w['dhead'], dev), _up(w['a2'], dev), _up(w['w_heads'], dev)
    wt, bias = _up(w['enc_wt'], dev), _up(w['enc_bias'], dev)
    table = env.encode_table(wt) if cfg.get('table') else None
    for k in range(cfg.get('windows', 1)):
        x1, dz, de = (torch.full((T, R, H), float('nan'), device=dev) for _ in range(3))
        parts = torch.full((ops.mlp_backward_partials(T * R, H), H), float('nan'), device=dev)
        ops.mlp_backward(env, T, E, N, H, h, dhead, snaps, wt, bias, a2, w_heads, x1, dz, de, parts, loc_table=table,
                         enc_first=(k == 0), enc_window=cfg.get('enc_window', True), a2_grad=a2g)
    torch.cuda.synchronize()
    return dict(x1=x1, dz=dz, de=de, parts=parts, a2g=a2g, a2g0=a2g0)


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_mlp_window_backward_against_float64(name):
    """The x1 / dz / de rings, the partials from a NaN pre-fill (their column sum; every row where there is one per tile), a2_grad
    on top of its pre-fill, the encoder's dWt / db through the finishes that go with the form (window form: ordered and plain) —
    against the float64 window backward, each at its bar; then the same call(s) again on fresh copies: the rings, the partials and
    a2_grad the same bits."""
    from ic3net_amd import ops
    cfg = MLP_CASES[name]
    env = cfg['env']()
    T, H, OT = cfg['T'], cfg['H'], cfg.get('OT', 6)
    E, N = env.nenvs, env.nagents_env
    Q = T * E * N
    assert ops.mlp_backward_supported(env, H)
    tiles = (Q + 63) // 64
    if cfg.get('walk'):
        assert ops.mlp_backward_partials(Q, H) < tiles
    else:
        assert ops.mlp_backward_partials(Q, H) == tiles
    windows, enc_window = cfg.get('windows', 1), cfg.get('enc_window', True)
    w = ref.make_mlp_window(sum(map(ord, name)), T, E, N, H, OT, env.obs_dim)
    snaps, obs = _record_states(env, T)
    want = ref.mlp_reference_of(w, obs)
    got = _launch_mlp(env, w, cfg, snaps)
    errs = ref.mlp_errors(want, _num(got['x1']), _num(got['dz']), _num(got['de']), _num(got['parts']), _num(got['a2g']),
                          _num(got['a2g0']), windows=windows)
    assert ('dbias_tiles' in errs) == (not cfg.get('walk'))
    finishes = [('_ordered', env.encode_backward_window_finish_ordered), ('', env.encode_backward_window_finish)] if enc_window \
        else [('', env.encode_backward_finish)]
    for tag, fin in finishes:
        dwt, db = fin(H)
        errs['enc_dwt' + tag] = ref.rel_err(_num(dwt), windows * want['enc_dwt'])
        errs['enc_db' + tag] = ref.rel_err(_num(db), windows * want['enc_db'])
    again = _launch_mlp(env, w, cfg, snaps)
    for k in ('x1', 'dz', 'de', 'parts', 'a2g'):
        assert torch.equal(got[k], again[k]), k
    ref.check('gpu/' + name, errs)

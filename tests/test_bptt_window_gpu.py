"""GPU: ic3_bptt_backward (ops.bptt_backward) — the LSTM window backward as ONE host call — against the float64 window backward of
tests/bptt_window_ref.py on synthetic records: the detach points, the row factors of collection mode, the two chains' offsets into
every buffer (two streams), NULL mask entries, the ring and the one-buffer form of dxh, and a chain whose communication backward
runs more than one round of its persistent grid.  Every case is launched a second time on fresh copies: bit-identical."""
import numpy as np
import pytest
import torch

import bptt_window_ref as ref

pytestmark = pytest.mark.gpu


def _pp(N, dim, vision, E):
    from test_env_parity_gpu import make_pp
    return make_pp(N, dim, vision, 'mixed', E, seed=3)


def _tj(N, dim, difficulty, E):
    from test_env_parity_gpu import make_tj
    return make_tj(N, dim, 1, difficulty, E, seed=3, add_rate_min=0.5, add_rate_max=0.5)


CASES = {
    'h128-pp-hard-E131-T5-gap2-ring-two-chains': dict(env=lambda: _pp(10, 20, 1, 131), H=128, T=5, gap=2, ring=True),
    'h128-tj-hard-E67-T4-gap2-one-buffer': dict(env=lambda: _tj(20, 18, 'hard', 67), H=128, T=4, gap=2, ring=False, alive='first_null'),
    'h64-pp-n3-E200-T6-collect-sum-ring-two-chains': dict(env=lambda: _pp(3, 6, 1, 200), H=64, T=6, collect=True, avg=False, ring=True,
                                                         alive='all'),
    'h64-tj-n5-E130-T4-collect-comm-zero': dict(env=lambda: _tj(5, 6, 'easy', 130), H=64, T=4, collect=True, comm_zero=True, ring=True),
    # 32 agents need 33 cells: dim 6 is the smallest grid ic3_pp_create takes, and the window backward runs on it at hid 256
    'h256-pp-n32-dim6-E130-T3-gap3': dict(env=lambda: _pp(32, 6, 1, 130), H=256, T=3, gap=3, ring=True),
    # E1 = 1536 envs = 512 tiles of 3 on 512 slots | 1564 envs = 522 tiles = 2 rounds of 261 workgroups (no encoder share here)
    'h128-tj-hard-E3100-T2-two-rounds': dict(env=lambda: _tj(20, 18, 'hard', 3100), H=128, T=2, gap=0, ring=True, alive='all',
                                             encoder=False, slots=512 + 261),
}


def _launch(env, w, dev, cfg, snaps, two):
    """One ic3_bptt_backward on fresh device copies; returns the buffers it wrote (NaN-filled / pre-filled with known values)."""
    from ic3net_amd import ops
    T, E, N, H = w['T'], w['E'], w['N'], w['H']
    R = E * N
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    ups = lambda ms: None if ms is None else [up(m) for m in ms]
    gates, dh, dc = up(w['gates']), up(w['dh']), up(w['dc'])
    dxh = torch.full((T, R, 2 * H) if cfg['ring'] else (R, 2 * H), float('nan'), device=dev)
    g = torch.Generator().manual_seed(99)
    bias0 = torch.randn(((R + 63) // 64, 4 * H), generator=g)
    comm_zero = cfg.get('comm_zero', False)
    slots = ops.bptt_dcw_partials(E, N, two)
    dcw0 = torch.randn((slots, H, H), generator=g)
    bias, dcw = bias0.to(dev), dcw0.to(dev)
    wb3 = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh']))
    ops.bptt_backward(env, T, E, N, H, gates, up(w['hs']), up(w['cs']), up(w['dhead']), snaps, ups(w['alive']), ups(w['gate']), wb3,
                      up(w['w_heads']), up(w['c_weight']), dh, dc, dxh, bias, None if comm_zero else dcw,
                      mode_avg=cfg.get('avg', True), comm_zero=comm_zero, detach_gap=cfg.get('gap', 0), row_live=up(w['row_live']),
                      row_keep=up(w['row_keep']), enc_first=True, two_chains=two)
    torch.cuda.synchronize()
    return dict(gates=gates, dh=dh, dc=dc, dxh=dxh, bias=bias, dcw=dcw, bias0=bias0, dcw0=dcw0, slots=slots)


@pytest.mark.parametrize("name", list(CASES))
def test_window_backward_against_float64(name):
    """dgates and the dxh ring of every step (the last-written step in the one-buffer form), dh / dc leaving the window, every row of
    the bias partials, the sum over the dcw slots and their count, the encoder's dWt / db through the finish that goes with the form,
    ic3_lstm_weight_grad on the in-place record (hid 64 / 128) — against the float64 window backward, each at its bar
    (bptt_window_ref.check); then the same call again on fresh copies: dgates, dh, dc and both partial buffers the same bits (the two
    chains share them across two streams: a race would show)."""
    from ic3net_amd import ops
    cfg = CASES[name]
    env = cfg['env']()
    dev = env.device
    T, H, OT = cfg['T'], cfg['H'], 6
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.bptt_backward_supported(env, H)
    two = cfg['ring'] and ops.first_chain_envs(E, N) < E
    assert two == (cfg['ring'] and E >= 128)
    w = ref.make_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False), alive=cfg.get('alive', 'none'))
    rng = np.random.default_rng(7)
    env.reset()
    snaps = torch.empty((T, env.dims.state_words), dtype=torch.int32, device=dev)
    obs = []
    for t in range(T):
        for _ in range(2):
            env.step(rng.integers(0, env.dims.naction, (E, N)), observe=False)
        env.snapshot(out=snaps[t])
        if cfg.get('encoder', True):
            obs.append(env.observe().reshape(R, env.obs_dim).double().cpu().numpy())
    want = ref.reference_of(w, obs=obs or None, detach_gap=cfg.get('gap', 0), mode_avg=cfg.get('avg', True),
                            comm_zero=cfg.get('comm_zero', False))
    got = _launch(env, w, dev, cfg, snaps, two)
    num = lambda v: v.double().cpu().numpy()
    errs = dict(dgates=ref.rel_err(num(got['gates']), want['dgates']), dh=ref.rel_err(num(got['dh']), want['dh']),
                dc=ref.rel_err(num(got['dc']), want['dc']))
    errs['dxh'] = ref.rel_err(num(got['dxh']), want['dxh'] if cfg['ring'] else want['dxh'][0])
    errs['dbias_rows'] = ref.rel_err(num(got['bias']), num(got['bias0']) + want['dbias_rows'])
    if cfg.get('comm_zero', False):
        assert torch.equal(got['dcw'].cpu(), got['dcw0'])
    else:
        assert got['slots'] == cfg.get('slots', got['slots'])
        errs['dcw'] = ref.rel_err(num(got['dcw']).sum(0), num(got['dcw0']).sum(0) + want['dcw'])
    if obs:
        dwt, db = env.encode_backward_window_finish(H) if cfg['ring'] else env.encode_backward_finish(H)
        errs['enc_dwt'], errs['enc_db'] = ref.rel_err(num(dwt), want['enc_dwt']), ref.rel_err(num(db), want['enc_db'])
    if H != 256:                                                 # (ic3_lstm_weight_grad: hid 64 / 128)
        dW0 = torch.randn((2 * H, 4 * H), generator=torch.Generator().manual_seed(5))
        dW = dW0.to(dev)
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        ops.lstm_weight_grad(up(w['inp']), up(w['hs']), got['gates'], dW, row_live=up(w['row_live']))
        errs['dW'] = ref.rel_err(num(dW), num(dW0) + want['dW'])
    again = _launch(env, w, dev, cfg, snaps, two)
    for k in ('gates', 'dh', 'dc', 'bias', 'dcw'):
        assert torch.equal(got[k], again[k]), k
    ref.check('gpu/' + name, errs)


def test_a_refused_window_leaves_the_record_alone():
    """detach_gap > 0 together with row_keep: ValueError naming both, before any launch — gates, dh, dc and the partials keep their bits."""
    from ic3net_amd import ops
    env = _pp(3, 6, 1, 130)
    dev = env.device
    env.reset()
    w = ref.make_window(1, 3, 130, 3, 64, 6, collect=True)
    snaps = torch.stack([env.snapshot() for _ in range(3)])
    cfg = dict(ring=True, gap=2)
    with pytest.raises(ValueError, match="detach_gap.*row_keep"):
        _launch(env, w, dev, cfg, snaps, True)
    # (the buffers of the refused call are gone with the exception: once more by hand, keeping them)
    up = lambda a: torch.from_numpy(a).to(dev)
    gates, dh, dc = up(w['gates']), up(w['dh']), up(w['dc'])
    bias, dcw = torch.ones((7, 256), device=dev), torch.ones((ops.bptt_dcw_partials(130, 3, True), 64, 64), device=dev)
    dxh = torch.full((3, 390, 128), float('nan'), device=dev)
    wb3 = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh']))
    with pytest.raises(ValueError):
        ops.bptt_backward(env, 3, 130, 3, 64, gates, up(w['hs']), up(w['cs']), up(w['dhead']), snaps, None, [up(m) for m in w['gate']],
                          wb3, up(w['w_heads']), up(w['c_weight']), dh, dc, dxh, bias, dcw, detach_gap=2, row_live=up(w['row_live']),
                          row_keep=up(w['row_keep']), two_chains=True)
    torch.cuda.synchronize()
    assert torch.equal(gates.cpu(), torch.from_numpy(w['gates'])) and torch.equal(dh.cpu(), torch.from_numpy(w['dh']))
    assert torch.equal(dc.cpu(), torch.from_numpy(w['dc'])) and bool((bias == 1).all()) and bool((dcw == 1).all())
    assert bool(torch.isnan(dxh).all())

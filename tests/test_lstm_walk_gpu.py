"""GPU: ops.bptt_backward(walk=True) — ic3_bptt_backward on an ic3_bptt_walk descriptor, a comm_zero window of the LSTM backward
through time with its T steps walked in ONE launch (lstm_gates_bwd_walk_kernel<64 / 128 / 256>) — against walk=False (a gate launch
and the copy of d h_prev per step and chain) on the same inputs, with BOTH two_chains settings on the per-step side (a chain border
never splits a 64-row tile, so the bias rows correspond): the gate record (dgates), the d inp columns of every ring slot, dh and dc
leaving the window, every row of the bias partials (pre-filled: they are added to) and the encoder's dWt / db through the window form's
ordered finish — BIT FOR BIT; the d h_prev columns of the walk's ring keep their NaN pre-fill.  Shapes: the existing comm-zero shape
(TJ-easy, collection cuts), PP-hard E = 131 at hid 128 (also with max_workgroups = 3: a workgroup walks 7 tiles), 32 agents at hid
256, and 513 tiles at hid 64, more than the launch has workgroups at the library's own plan.  Every case is launched a second time on
fresh copies: bit-identical."""
import numpy as np
import pytest
import torch

import bptt_window_ref as ref
from test_bptt_window_gpu import _pp, _tj

pytestmark = pytest.mark.gpu

CASES = {
    'h64-tj-n5-E130-T4-collect': dict(env=lambda: _tj(5, 6, 'easy', 130), H=64, T=4, collect=True),
    'h128-pp-n10-dim20-E131-T5-gap2': dict(env=lambda: _pp(10, 20, 1, 131), H=128, T=5, gap=2),
    'h128-pp-n10-dim20-E131-T5-gap2-three-workgroups': dict(env=lambda: _pp(10, 20, 1, 131), H=128, T=5, gap=2, wgs=3),
    'h256-pp-n32-dim6-E130-T3-gap3': dict(env=lambda: _pp(32, 6, 1, 130), H=256, T=3, gap=3),
    # 32 800 rows = 513 tiles (the last one half full) on the 512 workgroup slots of hid 64: workgroup 0 walks tiles 0 and 512
    'h64-tj-n5-E6560-T2-513-tiles': dict(env=lambda: _tj(5, 6, 'easy', 6560), H=64, T=2, gap=0, tiles=513),
}


def _launch(env, w, cfg, snaps, walk, two=False):
    """One ops.bptt_backward (comm_zero, the ring) on fresh device copies, and the encoder's ordered window finish behind it."""
    from ic3net_amd import ops
    dev = env.device
    T, E, N, H = w['T'], w['E'], w['N'], w['H']
    R = E * N
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    gates, dh, dc = up(w['gates']), up(w['dh']), up(w['dc'])
    dxh = torch.full((T, R, 2 * H), float('nan'), device=dev)
    bias = torch.randn(((R + 63) // 64, 4 * H), generator=torch.Generator().manual_seed(99)).to(dev)
    wb3 = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh']))
    ops.bptt_backward(env, T, E, N, H, gates, up(w['hs']), up(w['cs']), up(w['dhead']), snaps, None, None, wb3, up(w['w_heads']), None,
                      dh, dc, dxh, bias, None, comm_zero=True, detach_gap=cfg.get('gap', 0), row_live=up(w['row_live']),
                      row_keep=up(w['row_keep']), enc_first=True, two_chains=two, walk=walk, max_workgroups=cfg.get('wgs', 0) if walk else 0)
    dwt, db = [v.clone() for v in env.encode_backward_window_finish_ordered(H)]
    torch.cuda.synchronize()
    return dict(dgates=gates, dh=dh, dc=dc, dinp=dxh[..., :H].contiguous(), bias=bias, enc_dwt=dwt, enc_db=db), dxh[..., H:]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_walk_against_the_per_step_call(name):
    from ic3net_amd import ops
    cfg = CASES[name]
    env = cfg['env']()
    dev = env.device
    T, H, OT = cfg['T'], cfg['H'], 6
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.bptt_backward_supported(env, H)
    tiles = (R + 63) // 64
    assert tiles == cfg.get('tiles', tiles) and tiles > cfg.get('wgs', 0)
    w = ref.make_window(sum(map(ord, name)), T, E, N, H, OT, collect=cfg.get('collect', False))
    rng = np.random.default_rng(7)
    env.reset()
    snaps = torch.empty((T, env.dims.state_words), dtype=torch.int32, device=dev)
    for t in range(T):
        for _ in range(2):
            env.step(rng.integers(0, env.dims.naction, (E, N)), observe=False)
        env.snapshot(out=snaps[t])
    walk, walk_dhp = _launch(env, w, cfg, snaps, walk=True)
    assert bool(torch.isnan(walk_dhp).all()) and not bool(torch.isnan(walk['dinp']).any())
    assert not torch.equal(walk['dgates'].cpu(), torch.from_numpy(w['gates']))
    assert ops.first_chain_envs(E, N) < E                        # (the second setting does run two chains at these sizes)
    for two in (False, True):
        steps, steps_dhp = _launch(env, w, cfg, snaps, walk=False, two=two)
        assert not bool(torch.isnan(steps_dhp).any())
        bad = [k for k in steps if not _same_bits(steps[k], walk[k])]
        for k in bad:                                            # (each figure in front of the assertion)
            print("lstm-walk gpu/%s two_chains=%d %s: max |walk - per-step| %.3e" % (name, two, k, (steps[k] - walk[k]).abs().max().item()))
        assert not bad, "%s (two_chains=%d): the walk differs from the per-step call in %r" % (name, two, bad)
    again, _ = _launch(env, w, cfg, snaps, walk=True)
    for k in walk:
        assert _same_bits(walk[k], again[k]), k
